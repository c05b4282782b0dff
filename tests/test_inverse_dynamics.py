"""Inverse dynamics and bias accelerations on the device (dexsim_inverse_dynamics, dexsim_body_bias_accel) against
tests/invdyn_ref.py: the fp64 CPU oracle's M(q) qdd + b(q, qd) (its bias b includes gravity; a second oracle pair built from a
zero-gravity config gives the velocity-product force c(q, qd) directly), and a float64 numpy recursion for Jdot qd.

Inputs: poses from HandKin.random_poses (the full joint range), qd uniform in +-3 (m/s on the slides, rad/s otherwise), qdd uniform
in +-10, all rounded to float32.  +-3 is deliberate: at +-1 the velocity-product force is about 0.2 % of gravity in the scaled metric
E_tau, at +-3 about 2 %, so a wrong Coriolis term cannot hide under the gravity force.

Metrics (invdyn_ref.err_tau, err_acc): E_tau has kindyn_ref.err_g's form -- per pose max_j |tau - tau64|_j / sqrt(M64_jj) over
max_j |tau64|_j / sqrt(M64_jj), then the max over poses.  E_acc is per pose, linear and angular rows separately, the maximum
absolute error over bodies over the maximum absolute reference value of the pose.

Tolerances: 4 x the same figure of the fp32 reference against the fp64 reference on the SAME poses -- the fp32 oracle's
M32 @ qdd + b32 formed in float32, the float32 run of the numpy recursion.  The factor 4 is test_kindyn.py's, with its reasons: the
project's factor 3 for "a different factorisation of the same fp32 arithmetic" plus one for sincos_joint and the 2.5-ulp division /
root of the build.  test_reference_roundoff caps 4 x every figure at 1e-3 on 300 poses; any sign, index, lever or dropped-term error
is >= 1e-2.  Measured on one MI355X (profiles/inverse_dynamics/README.md has the full list): E_tau 4.85e-7 full, 2.89e-7 bias,
1.07e-6 velocity-product (fp32 oracle 1.25e-5, 7.5e-7, 4.93e-6); E_acc 1.04e-6 linear, 4.6e-7 angular (float32 recursion 2.6e-6,
2.93e-7).  The angular rows are the tight ones -- they carry the direction error of joint_frame's axes (sincos_joint) with no lever to
average over: on the scaled model 1.05e-6 against a bound of 1.06e-6.  Every GPU test uses N = 70: two workgroups, six live lanes in the second.  Every device output sits between two guard
rows that must come back untouched.
"""
import ctypes as C

import numpy as np
import pytest

from dexrobot_isaac_amd import _abi
from oracle.oracle import Oracle
from tests import invdyn_ref as ir
from tests import kindyn_ref as kr
from tests.query_rig import (bits, dev as _dev, guarded as _guarded, guards_ok as _guards_ok, load_lib, pose_core, purity_frame,
                             setup as _setup, stub_core)

N = 70
NB, NJ = _abi.NUM_HAND_BODIES, _abi.NJ
FACTOR = ir.FACTOR


# ------------------------------------------------------------------------------------------------- CPU
@pytest.fixture(scope="module")
def lib():
    return load_lib()


def test_abi_exports_and_null_handle(lib):
    for name in ("dexsim_inverse_dynamics", "dexsim_body_bias_accel"):
        assert name in _abi.EXPORTED_SYMBOLS
        assert hasattr(lib, name), f"libdexsim.so does not export {name}"
    assert lib.dexsim_inverse_dynamics(None, None, 1, None, None, None, 1, None, None) == 1  # DEXSIM_ERR_ARG
    assert b"null handle" in lib.dexsim_last_error()
    assert lib.dexsim_body_bias_accel(None, None, 1, None, None, None, NB, None, None) == 1
    assert b"null handle" in lib.dexsim_last_error()


def references(sc, ms, q, qd, qdd):
    """Every reference of the poses (q, qd, qdd), computed once: the oracle pairs with and without gravity, the float64 and float32
    runs of the Jdot qd recursion, and the fp32-against-fp64 figures the tolerances are 4 x of."""
    hk = kr.HandKin(ms)
    o32, o64 = kr.oracle_pair(sc, ms)
    sc0 = ir.zero_gravity_config(sc.num_envs)
    z32, z64 = Oracle(sc0, ms, f64=False), Oracle(sc0, ms, f64=True)
    M64, b64 = ir.mass_bias(o64, q, qd)
    M32, b32 = ir.mass_bias(o32, q, qd)
    _, c64 = ir.mass_bias(z64, q, qd)
    _, c32 = ir.mass_bias(z32, q, qd)
    _, g64 = kr.mass_gravity(o64, q)
    _, g32 = kr.mass_gravity(o32, q)
    full64 = ir.tau_of(M64, b64, qdd)
    acc64 = np.stack([ir.bias_accel(hk, x.astype(np.float64), v.astype(np.float64)) for x, v in zip(q, qd)])
    acc32 = np.stack([ir.bias_accel(hk, x, v, np.float32) for x, v in zip(q, qd)])
    e_lin, e_ang = ir.err_acc(acc32, acc64)
    return dict(hk=hk, q=q, qd=qd, qdd=qdd, M64=M64, b64=b64, c64=c64, g64=g64, full64=full64, acc64=acc64,
                e_full=ir.err_tau(ir.tau_of(M32, b32, qdd, np.float32), full64, M64), e_bias=ir.err_tau(b32.astype(np.float32), b64, M64),
                e_c=ir.err_tau(c32.astype(np.float32), c64, M64), e_g=kr.err_g(g32, g64, M64), e_M=kr.err_M(M32, M64),
                e_lin=e_lin, e_ang=e_ang)


def test_reference_roundoff():
    """The measurement the GPU tolerances rest on, and its cap.  Measured over these 300 poses: e_full = 2.33e-5, e_bias = 8.7e-7,
    e_c = 5.5e-6, e_lin = 4.1e-6, e_ang = 3.5e-7.  The GPU tests recompute the figures on their own 70 poses."""
    _reference_roundoff(None)


def test_reference_roundoff_generic_model():
    """The same measurement and cap on the model of tests/generic_model.py, every body on a frame of its own."""
    _reference_roundoff("generic")


def _reference_roundoff(model):
    sc, ms = _setup(1, model=model, free_bodies=model is not None)
    q = kr.HandKin(ms).random_poses(300, seed=3)
    qd, qdd = ir.random_rates(300, seed=4)
    r = references(sc, ms, q, qd, qdd)
    print("reference roundoff over 300 poses: " + ", ".join(f"{k} = {r[k]:.3g}" for k in ("e_full", "e_bias", "e_c", "e_lin", "e_ang")))
    for k in ("e_full", "e_bias", "e_c", "e_lin", "e_ang"):
        assert 0 < FACTOR * r[k] <= 1e-3, k


def test_reference_bias_accel_is_jdot_qd():
    """The Jdot qd recursion against central differences of HandKin.jacobian along qd, in float64:
    ((J(q + h qd) - J(q - h qd)) / 2h) @ qd with h = 1e-4.  What the step allows: along s -> q + s qd every entry of J is a
    trigonometric polynomial of total frequency <= W = sum |qd| over the revolute joints of the body's chain (the slides lie
    before every hinge, so they enter no lever) and of amplitude <= L, the lever (below 0.5 m; 1 for the angular rows), so the
    central difference of an entry is off by <= h^2 W^3 L / 6 and the product with qd by <= h^2 W^4 L / 6; roundoff of the
    difference quotient (1e-16 / h per entry) is far below that."""
    _, ms = _setup(1)
    hk = kr.HandKin(ms)
    h = 1e-4
    q = hk.random_poses(8, seed=5).astype(np.float64)
    qd = ir.random_rates(8, seed=6)[0].astype(np.float64)
    worst = 0.0
    for x, v in zip(q, qd):
        fd = np.einsum("bdj,j->bd", (hk.jacobian(x + h * v) - hk.jacobian(x - h * v)) / (2 * h), v)
        acc = ir.bias_accel(hk, x, v)
        W = np.abs(v[3:6]).sum() + np.abs(v[6:]).reshape(5, 4).sum(1).max()
        e_lin, e_ang = np.abs(acc[:, 0:3] - fd[:, 0:3]).max(), np.abs(acc[:, 3:6] - fd[:, 3:6]).max()
        b_lin, b_ang = h * h * W ** 4 * 0.5 / 6, h * h * W ** 4 * 1.0 / 6
        print(f"Jdot qd against central differences: linear {e_lin:.3g} (bound {b_lin:.3g}, scale {np.abs(fd[:, 0:3]).max():.3g}), "
              f"angular {e_ang:.3g} (bound {b_ang:.3g}, scale {np.abs(fd[:, 3:6]).max():.3g})")
        assert e_lin <= b_lin and e_ang <= b_ang
        # the bound is small against the quantity itself: a wrong or missing term could not pass
        assert b_lin < 1e-3 * np.abs(fd[:, 0:3]).max() and b_ang < 1e-3 * np.abs(fd[:, 3:6]).max()
        worst = max(worst, e_lin, e_ang)
    assert worst > 0


def test_velocity_terms_are_discriminated():
    """The fp64 gravity force alone (qd = 0) in place of the bias force at qd in +-3 misses the bound by at least 100 x: a kernel
    that dropped the velocity-product terms could not pass."""
    sc, ms = _setup(1)
    q = kr.HandKin(ms).random_poses(N, seed=21)
    qd, qdd = ir.random_rates(N, seed=31)
    r = references(sc, ms, q, qd, qdd)
    miss = ir.err_tau(r["g64"], r["b64"], r["M64"])
    print(f"gravity force alone against the bias force: E_tau = {miss:.3g}, the bound is {FACTOR * r['e_bias']:.3g}")
    assert miss >= 100 * FACTOR * r["e_bias"]


_stub_core = stub_core(dict(
    inverse_dynamics=lambda tau, qdd=None, env_ids=None, q=None, qd=None, gravity=True:
        ("tau", tuple(tau.shape), qdd is not None, q is not None, qd is not None, gravity),
    body_bias_accel=lambda out, env_ids=None, q=None, qd=None, bodies=None: ("acc", tuple(out.shape), bodies),
    body_jacobian=lambda out, env_ids=None, q=None, bodies=None: ("jac", tuple(out.shape), bodies)))


def test_env_argument_validation():
    import torch
    from dexrobot_isaac_amd import make_env
    from oracle.py_backend import OracleCore
    env = make_env("BaseTask", 3, "cpu", "cpu", 0, _core_factory=_stub_core)
    z = lambda *s: torch.zeros(*s)
    for call in (env.get_inverse_dynamics, env.get_bias_forces, env.get_body_bias_acceleration):
        with pytest.raises(ValueError, match="q and qd"):
            call(q=z(4, NJ))                                                    # q without qd
        with pytest.raises(ValueError, match="q and qd"):
            call(qd=z(3, NJ))                                                   # qd without q
        with pytest.raises(ValueError, match="shape"):
            call(q=z(4, NJ), qd=z(5, NJ))
        with pytest.raises(ValueError, match="shape"):
            call(q=z(4, NJ - 1), qd=z(4, NJ - 1))
        with pytest.raises(ValueError, match="out"):
            call(out=z(4, NJ))
    with pytest.raises(ValueError, match="shape"):
        env.get_inverse_dynamics(qdd=z(4, NJ))                                  # three envs
    with pytest.raises(ValueError, match="shape"):
        env.get_inverse_dynamics(qdd=z(3, NJ), env_ids=[0, 2])                  # qdd goes with the output rows
    with pytest.raises(ValueError, match="unknown body"):
        env.get_body_bias_acceleration(bodies=["r_f_link9_tip"])
    with pytest.raises(ValueError, match="body index"):
        env.get_body_bias_acceleration(bodies=[NB])
    with pytest.raises(ValueError, match="get_jacobian: unknown body"):        # the shared helper keeps get_jacobian's messages
        env.get_jacobian(bodies=["r_f_link9_tip"])
    assert not env._core.calls                                                 # nothing reached the core
    assert env.get_inverse_dynamics(qdd=z(2, NJ), env_ids=[2, 0], gravity=False).shape == (2, NJ)
    assert env._core.calls[-1] == ("tau", (2, NJ), True, False, False, False)
    assert env.get_bias_forces(q=z(5, NJ), qd=z(5, NJ)).shape == (5, NJ)
    assert env._core.calls[-1] == ("tau", (5, NJ), False, True, True, True)
    assert env.get_body_bias_acceleration(bodies=["r_f_link2_tip", 6]).shape == (3, 2, 6)
    assert env._core.calls[-1] == ("acc", (3, 2, 6), [18, 6])
    plain = make_env("BaseTask", 2, "cpu", "cpu", 0, _core_factory=OracleCore)  # the CPU stand-in has no such tensors
    for call in (plain.get_inverse_dynamics, plain.get_bias_forces, plain.get_body_bias_acceleration):
        with pytest.raises(NotImplementedError):
            call()


# ------------------------------------------------------------------------------------------------- GPU helpers
gpu_tau, check_tau = ir.gpu_tau, ir.check_tau


def gpu_acc(core, k, env_ids=None, q=None, qd=None, bodies=None):
    full, out = _guarded(k, NB if bodies is None else len(bodies), 6)
    core.body_bias_accel(out, env_ids=env_ids, q=_dev(q), qd=_dev(qd), bodies=bodies)
    _guards_ok(full)
    return out.cpu().numpy()


def gpu_mass(core, k, q=None):
    fm, M = _guarded(k, NJ, NJ)
    fg, g = _guarded(k, NJ)
    core.mass_matrix(mass=M, gravity=g, q=_dev(q))
    _guards_ok(fm)
    _guards_ok(fg)
    return M.cpu().numpy(), g.cpu().numpy()


def _case(ms, sc, seed):
    """A core of N envs posed at (q, qd) and every reference the tests share."""
    from dexrobot_isaac_amd.core import DexSimCore
    core = DexSimCore(sc, ms, "cuda:0")
    core.reset()
    q = kr.HandKin(ms).random_poses(N, seed)
    qd, qdd = ir.random_rates(N, seed + 10)
    pose_core(core, q, qd=qd)
    assert (core.field("qd").t().cpu().numpy() == qd).all()
    return dict(references(sc, ms, q, qd, qdd), core=core, sc=sc)


@pytest.fixture(scope="module")
def posed():
    sc, ms = _setup(N)
    c = _case(ms, sc, seed=21)
    core = c["core"]
    c["full"] = gpu_tau(core, N, qdd=c["qdd"])
    c["bias"] = gpu_tau(core, N)
    c["vel"] = gpu_tau(core, N, gravity=False)
    c["acc"] = gpu_acc(core, N)
    return c


def check_acc(acc, acc64, e_lin, e_ang, what):
    assert not np.isnan(acc).any(), f"{what}: an element was not written"
    E_lin, E_ang = ir.err_acc(acc, acc64)
    print(f"{what}: E_acc linear = {E_lin:.3g} (float32 recursion: {e_lin:.3g}, bound {FACTOR * e_lin:.3g}), "
          f"angular = {E_ang:.3g} (float32 recursion: {e_ang:.3g}, bound {FACTOR * e_ang:.3g})")
    assert E_lin <= FACTOR * e_lin and E_ang <= FACTOR * e_ang
    assert (bits(acc[:, 0]) == 0).all()                                        # hand_mount: +0.0f everywhere


def check_all(c, full, bias, vel, acc, what):
    check_tau(full, c["full64"], c["M64"], c["e_full"], f"{what}, full (qdd, gravity)")
    check_tau(bias, c["b64"], c["M64"], c["e_bias"], f"{what}, bias force (gravity)")
    check_tau(vel, c["c64"], c["M64"], c["e_c"], f"{what}, velocity-product force (no gravity)")
    check_acc(acc, c["acc64"], c["e_lin"], c["e_ang"], what)


# ------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_tau_against_fp64_oracle(posed):
    c = posed
    check_tau(c["full"], c["full64"], c["M64"], c["e_full"], "full (qdd, gravity)")
    check_tau(c["bias"], c["b64"], c["M64"], c["e_bias"], "bias force (gravity)")
    check_tau(c["vel"], c["c64"], c["M64"], c["e_c"], "velocity-product force (no gravity)")
    slides = np.zeros_like(c["qd"])
    slides[:, 0:3] = c["qd"][:, 0:3]                                            # only the three slides move: nothing turns
    only = gpu_tau(c["core"], N, q=c["q"], qd=slides, gravity=False)
    assert (only == 0).all()


@pytest.mark.gpu
def test_consistency_on_the_device(posed):
    """tau(full) - tau(bias) against M_dev @ qdd, and tau(qd = 0, gravity) against the gravity output of dexsim_mass_matrix.
    Bounds, in E_tau's per-joint scaling d_j = sqrt(M64_jj): each side is within 4 x its fp32-oracle figure of the fp64 value, so
    the two differ by at most the sum -- 4 (e_full S_full + e_bias S_bias) + sum_i 4 e_M d_i |qdd_i| for the first (S = the pose's
    max_j |tau64|_j / d_j; |M_dev - M64|_ji <= 4 e_M d_j d_i is test_kindyn's bound), 8 e_g S_g for the second."""
    c = posed
    M, g = gpu_mass(c["core"], N)
    d = np.sqrt(np.einsum("nii->ni", c["M64"]))
    S = lambda t: (np.abs(t) / d).max(1)
    qdd = c["qdd"].astype(np.float64)
    lhs = c["full"].astype(np.float64) - c["bias"].astype(np.float64)
    err = (np.abs(lhs - np.einsum("nij,nj->ni", M.astype(np.float64), qdd)) / d).max(1)
    bound = FACTOR * (c["e_full"] * S(c["full64"]) + c["e_bias"] * S(c["b64"]) + c["e_M"] * (d * np.abs(qdd)).sum(1))
    print(f"tau(full) - tau(bias) against M_dev @ qdd: worst error / bound = {(err / bound).max():.3g}")
    assert (err <= bound).all()
    rest = gpu_tau(c["core"], N, q=c["q"], qd=np.zeros_like(c["qd"]))
    err = (np.abs(rest.astype(np.float64) - g.astype(np.float64)) / d).max(1)
    bound = 2 * FACTOR * c["e_g"] * S(c["g64"])
    print(f"tau(qd = 0, gravity) against the gravity force of dexsim_mass_matrix: worst error / bound = {(err / bound).max():.3g}")
    assert (err <= bound).all()
    check_tau(rest, c["g64"], c["M64"], c["e_g"], "tau at rest against the fp64 gravity force")


@pytest.mark.gpu
def test_bias_accel_against_float64_recursion(posed):
    c = posed
    check_acc(c["acc"], c["acc64"], c["e_lin"], c["e_ang"], "default model")
    still = gpu_acc(c["core"], N, q=c["q"], qd=np.zeros_like(c["qd"]))
    assert (still == 0).all()                                                  # nothing moves: no bias acceleration
    slides = np.zeros_like(c["qd"])
    slides[:, 0:3] = c["qd"][:, 0:3]
    assert (gpu_acc(c["core"], N, q=c["q"], qd=slides) == 0).all()


@pytest.mark.gpu
def test_different_model():
    """Per-joint scaled offsets, centres of mass and masses, finger links with off-diagonal inertia (test_kindyn's model): no
    constant of the default model is baked in."""
    sc, ms = _setup(N, model="scaled")
    c = _case(ms, sc, seed=22)
    core = c["core"]
    check_all(c, gpu_tau(core, N, qdd=c["qdd"]), gpu_tau(core, N), gpu_tau(core, N, gravity=False), gpu_acc(core, N), "scaled model")
    core.close()


@pytest.mark.gpu
def test_structure_free_model():
    """The model of tests/generic_model.py, which has none of the default model's exact zeros, ones and repeated numbers, every
    body on a frame of its own: tau with and without qdd and gravity, the bias acceleration of all 37 bodies."""
    sc, ms = _setup(N, model="generic", free_bodies=True)
    c = _case(ms, sc, seed=23)
    core = c["core"]
    check_all(c, gpu_tau(core, N, qdd=c["qdd"]), gpu_tau(core, N), gpu_tau(core, N, gravity=False), gpu_acc(core, N), "generic model")
    core.close()


@pytest.mark.gpu
def test_addressing(posed):
    import torch
    c = posed
    core, q, qd, qdd = c["core"], c["q"], c["qd"], c["qdd"]
    ids = [69, 0, 64, 3, 63]
    assert (bits(gpu_tau(core, len(ids), env_ids=ids)) == bits(c["bias"][ids])).all()
    assert (bits(gpu_tau(core, len(ids), env_ids=ids, gravity=False)) == bits(c["vel"][ids])).all()
    assert (bits(gpu_tau(core, len(ids), env_ids=ids, qdd=qdd[ids])) == bits(c["full"][ids])).all()    # qdd rides with the output rows
    assert (bits(gpu_acc(core, len(ids), env_ids=ids)) == bits(c["acc"][ids])).all()
    assert (bits(gpu_tau(core, 1, env_ids=[37], qdd=qdd[[37]])) == bits(c["full"][[37]])).all()       # k = 1
    assert (bits(gpu_acc(core, 1, env_ids=[37])) == bits(c["acc"][[37]])).all()
    sel = [36, 6, 12, 0]                                                       # out of order
    assert (bits(gpu_acc(core, N, bodies=sel)) == bits(c["acc"][:, sel])).all()
    assert (bits(gpu_acc(core, len(ids), env_ids=ids, bodies=sel)) == bits(c["acc"][ids][:, sel])).all()
    # overrides, k = 130 (three workgroups): rows copied from env state are the state path's bits, the rest meet the reference
    n_new = 130 - N
    qn = c["hk"].random_poses(n_new, seed=23)
    vn, an = ir.random_rates(n_new, seed=24)
    src = np.concatenate([np.arange(40), np.full(n_new, -1), np.arange(40, N)])
    st = src >= 0
    cat = lambda old, new: np.concatenate([old[:40], new, old[40:]])
    qo, vo, ao = cat(q, qn), cat(qd, vn), cat(qdd, an)
    full = gpu_tau(core, 130, qdd=ao, q=qo, qd=vo, env_ids=[-1])               # env_ids is ignored with overrides
    bias, vel, acc = gpu_tau(core, 130, q=qo, qd=vo), gpu_tau(core, 130, q=qo, qd=vo, gravity=False), gpu_acc(core, 130, q=qo, qd=vo)
    for got, want in ((full, c["full"]), (bias, c["bias"]), (vel, c["vel"]), (acc, c["acc"])):
        assert (bits(got[st]) == bits(want[src[st]])).all()
    check_all(references(c["sc"], core.model, qn, vn, an), full[~st], bias[~st], vel[~st], acc[~st], "overrides")
    # ids outside [0, N) leave their rows as they are
    bad = [5, -1, N, 69]
    tb, ab = gpu_tau(core, 4, env_ids=bad, qdd=qdd[[5, 0, 0, 69]]), gpu_acc(core, 4, env_ids=bad, bodies=sel)
    assert np.isnan(tb[1:3]).all() and np.isnan(ab[1:3]).all()
    assert (bits(tb[[0, 3]]) == bits(c["full"][[5, 69]])).all() and (bits(ab[[0, 3]]) == bits(c["acc"][[5, 69]][:, sel])).all()
    # argument errors come back as DEXSIM_ERR_ARG with their message, before any launch
    lib, h = core.lib, core.h
    tau = torch.full((130, NJ), float("nan"), device=core.device)
    acc = torch.full((130, NB, 6), float("nan"), device=core.device)
    pt, pa = C.c_void_p(tau.data_ptr()), C.c_void_p(acc.data_ptr())
    pq, pv = C.c_void_p(_dev(qo).data_ptr()), C.c_void_p(_dev(vo).data_ptr())

    def refused(rc, text):
        assert rc == 1 and text in lib.dexsim_last_error(), (rc, lib.dexsim_last_error())
    refused(lib.dexsim_inverse_dynamics(h, None, 0, None, None, None, 1, pt, None), b"k must be positive")
    refused(lib.dexsim_inverse_dynamics(h, None, N - 1, None, None, None, 1, pt, None), b"k == num_envs")
    refused(lib.dexsim_inverse_dynamics(h, None, 130, pq, None, None, 1, pt, None), b"q and qd")
    refused(lib.dexsim_inverse_dynamics(h, None, N, None, pv, None, 1, pt, None), b"q and qd")
    refused(lib.dexsim_inverse_dynamics(h, None, N, None, None, None, 2, pt, None), b"flag")
    refused(lib.dexsim_inverse_dynamics(h, None, N, None, None, None, 1, None, None), b"tau")
    refused(lib.dexsim_body_bias_accel(h, None, 0, None, None, None, NB, pa, None), b"k must be positive")
    refused(lib.dexsim_body_bias_accel(h, None, N - 1, None, None, None, NB, pa, None), b"k == num_envs")
    refused(lib.dexsim_body_bias_accel(h, None, 130, pq, None, None, NB, pa, None), b"q and qd")
    refused(lib.dexsim_body_bias_accel(h, None, N, None, None, None, NB - 1, pa, None), b"bodies == NULL")
    refused(lib.dexsim_body_bias_accel(h, None, N, None, None, (C.c_int * 2)(3, NB), 2, pa, None), b"body index")
    refused(lib.dexsim_body_bias_accel(h, None, N, None, None, (C.c_int * 1)(3), 0, pa, None), b"nb must be")
    refused(lib.dexsim_body_bias_accel(h, None, N, None, None, None, NB, None, None), b"acc")
    torch.cuda.synchronize()
    assert torch.isnan(tau).all() and torch.isnan(acc).all()                   # nothing was launched


@pytest.mark.gpu
def test_purity():
    import torch
    qdd = ir.random_rates(N, seed=41)[1]
    rnd = lambda: torch.rand(100, NJ, device="cuda:0")

    def between(core):
        gpu_tau(core, 3, env_ids=[69, 1, 64], gravity=False)
        gpu_acc(core, 3, env_ids=[69, 1, 64], bodies=[12, 18])
        gpu_tau(core, 100, q=rnd(), qd=rnd(), qdd=rnd())
        gpu_acc(core, 100, q=rnd(), qd=rnd(), bodies=[6])
    t1, a1 = purity_frame(lambda core: [gpu_tau(core, N, qdd=qdd), gpu_acc(core, N)], between, n=N)
    assert not np.isnan(t1).any() and np.abs(a1).max() > 0                     # the stepped envs do move


@pytest.mark.gpu
def test_public_surface():
    import torch
    from dexrobot_isaac_amd import make_env
    env = make_env("BlindGrasping", N, "cuda:0", "cuda:0", 0)
    env.reset()
    g = torch.Generator().manual_seed(6)
    for _ in range(3):                                                         # some joint velocity
        env.step((2 * torch.rand(N, env.num_actions, generator=g) - 1).cuda())
    assert float(env.dof_vel.abs().max()) > 0
    qdd = (20 * torch.rand(N, NJ, generator=g) - 10).cuda()
    assert env.get_inverse_dynamics(qdd).shape == (N, NJ)                      # allocated by the call
    full, out = _guarded(N, NJ)
    tau = env.get_inverse_dynamics(qdd, out=out)
    _guards_ok(full)
    assert tau is out and not torch.isnan(tau).any()
    bias = env.get_bias_forces()
    assert bias.shape == (N, NJ) and torch.equal(bias.view(torch.int32), env.get_inverse_dynamics().view(torch.int32))
    assert not torch.equal(bias, env.get_bias_forces(gravity=False))
    assert torch.equal(env.get_bias_forces(env_ids=[3, 1]), bias[[3, 1]])
    tip = "r_f_link1_tip"
    assert env.get_body_bias_acceleration().shape == (N, NB, 6)
    full, out = _guarded(N, 1, 6)
    acc = env.get_body_bias_acceleration(bodies=[tip], out=out)
    _guards_ok(full)
    assert acc is out and not torch.isnan(acc).any()
    with pytest.raises(ValueError):
        env.get_body_bias_acceleration(bodies=["no_such_body"])
    with pytest.raises(ValueError):
        env.get_inverse_dynamics(q=env.dof_pos.clone())
    # the overrides at the current state: the state path's bits
    q0, v0 = env.dof_pos.clone(), env.dof_vel.clone()
    assert torch.equal(env.get_inverse_dynamics(qdd, q=q0, qd=v0).view(torch.int32), tau.view(torch.int32))
    assert torch.equal(env.get_body_bias_acceleration(bodies=[tip], q=q0, qd=v0).view(torch.int32), acc.view(torch.int32))
    # the operational-space identity on the device: J qdd + Jdot qd of the tip is the other call's row
    J = env.get_jacobian(bodies=[tip])
    xdd = torch.einsum("nbdj,nj->nbd", J, qdd) + acc
    assert xdd.shape == (N, 1, 6) and bool(torch.isfinite(xdd).all())
    env.close()
