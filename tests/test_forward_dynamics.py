"""Forward dynamics and mass-matrix solves on the device (dexsim_forward_dynamics, dexsim_mass_solve) against tests/fwddyn_ref.py:
qdd64 = solve(M64 [+ diag(a)], tau - b64) in float64, M64 and the bias force b64 = c + g from the fp64 CPU oracle (a zero-gravity
oracle pair gives c alone for the calls without the gravity flag).

Inputs: poses from HandKin.random_poses (the full joint range; the 70 poses of seed 21 as they come, every other draw through
fwddyn_ref.regular_poses, which skips draws within 6 degrees of the base's gimbal lock, where M is singular), qd from invdyn_ref.random_rates (+-3), a target acceleration y
uniform in +-10 and tau = float32(M64 y + b64), so that every joint's acceleration matters at its own scale; right-hand sides of the
mass solve are float32(M64 y) for y of the same kind.

Metrics (fwddyn_ref.err_qdd, err_res), with d_j = sqrt(M64_jj): E_qdd is per pose max_j |qdd - qdd64|_j d_j over max_j |qdd64|_j d_j,
then the max over poses -- invdyn_ref.err_tau's form with the dual scaling.  E_res = err_tau(M64 qdd + b64, tau, M64), the residual
as a force.  For the free acceleration tau is zero and err_tau would divide by zero: there the residual M64 qdd is measured against
the force that is there, -b64.  A column of the mass solve counts as a pose.

Tolerances: FACTOR = 4 x the same figure of the fp32 reference on the SAME poses -- fwddyn_ref.chol_solve run in float32 on the fp32
oracle's M32 and b32 -- recomputed by every test; test_kindyn.py gives the factor's reasons.  test_reference_roundoff caps 4 x every
figure at 1e-3 on 300 poses.  The figures are dominated by M32 against M64, not by the solve, so the device's different
factorisation (finger elimination, 6 x 6 Schur complement) has room under 4 x.

Every GPU test uses N = 70: two workgroups, six live lanes in the second; every device output sits between two guard rows that
must come back untouched.

Measured on one MI355X (profiles/forward_dynamics/README.md has the full list), device against fp32 reference: E_qdd 5.94e-05 /
5.56e-05 full, 7.02e-06 / 4.43e-05 free, 5.18e-05 / 6.49e-05 without flags, 4.79e-05 / 7.44e-05 mass solve; E_res 5.31e-07 /
5.90e-06, 3.72e-07 / 3.47e-06, 8.44e-07 / 7.44e-06, 9.38e-07 / 7.89e-06.  E_res is 4-15 x below the reference's; E_qdd is that
residual times the condition of the d-scaled M (1.6e3 here) and of the reference's size -- the full case is set by one pose 4.3
degrees from the base's gimbal lock.  On the scaled model with armature every figure is 3-8 x below the reference's.
"""
import ctypes as C

import numpy as np
import pytest

from dexrobot_isaac_amd import _abi
from oracle.oracle import Oracle
from tests import fwddyn_ref as fr
from tests import invdyn_ref as ir
from tests import kindyn_ref as kr
from tests.query_rig import (bits, dev as _dev, guarded as _guarded, guards_ok as _guards_ok, load_lib, pose_core, purity_frame,
                             setup as _setup, stub_core)

N = 70
NJ = _abi.NJ
FACTOR = 4
CASES = ("full", "free", "nograv", "msolve")


@pytest.fixture(scope="module")
def lib():
    return load_lib()


# ------------------------------------------------------------------------------------------------- references
def _as_poses(x, M64):
    """(n, r, 26) columns -> (n r, 26) poses with their M64."""
    x = np.asarray(x)
    return x.reshape(-1, NJ), np.repeat(M64, x.shape[1], axis=0)


def figures(x, c):
    """(E_qdd, E_res) of the solution x of case c (a dict of `references`)."""
    if c["cols"]:
        xp, Mp = _as_poses(x, c["M64"])
        x64p, rp = _as_poses(c["x64"], c["M64"])[0], _as_poses(c["force"], c["M64"])[0]
        return fr.err_qdd(xp, x64p, Mp), ir.err_tau(np.einsum("nij,nj->ni", Mp, xp.astype(np.float64)), rp, Mp)
    E = fr.err_qdd(x, c["x64"], c["M64"])
    if c["tau"] is None:
        return E, ir.err_tau(np.einsum("nij,nj->ni", c["M64"], np.asarray(x, dtype=np.float64)), c["force"], c["M64"])
    return E, fr.err_res(x, c["tau"], c["M64"], c["bias64"])


def references(sc, ms, q, qd, seed, arm=None, ncols=3):
    """Every reference of the poses (q, qd), computed once: per case the fp64 solution x64, the force it answers, and the
    fp32 reference's own figures (e_qdd, e_res) the tolerances are 4 x of.  arm: the armature the solve includes (float64)."""
    o32, o64 = kr.oracle_pair(sc, ms)
    sc0 = ir.zero_gravity_config(sc.num_envs)
    z32, z64 = Oracle(sc0, ms, f64=False), Oracle(sc0, ms, f64=True)
    M64, b64 = ir.mass_bias(o64, q, qd)
    M32, b32 = ir.mass_bias(o32, q, qd)
    _, c64 = ir.mass_bias(z64, q, qd)
    _, c32 = ir.mass_bias(z32, q, qd)
    n = len(q)
    y, tau = fr.targets(M64, b64, seed)
    _, tau0 = fr.targets(M64, c64, seed)
    ycol = np.random.default_rng(seed + 1).uniform(-10.0, 10.0, (n, ncols, NJ))
    rhs = np.einsum("nij,nrj->nri", M64, ycol).astype(np.float32)                      # (n, ncols, 26), as the device takes it
    A64 = M64 if arm is None else M64 + np.diag(arm)[None]
    A32 = (M32 if arm is None else M32 + np.diag(arm)[None]).astype(np.float32)
    f32 = np.float32
    out = dict(q=q, qd=qd, M64=M64, b64=b64, c64=c64, M32=M32, y=y, arm=arm, sc=sc, hk=kr.HandKin(ms),
               e_M=kr.err_M(M32, M64), e_id=ir.err_tau(ir.tau_of(M32, b32, y, f32), ir.tau_of(M64, b64, y), M64))
    spec = {"full": (tau, b64, b32), "free": (None, b64, b32), "nograv": (tau0, c64, c32)}
    for name, (t, bias64, bias32) in spec.items():
        force = -bias64 if t is None else t.astype(np.float64) - bias64
        force32 = -bias32.astype(f32) if t is None else t - bias32.astype(f32)
        c = dict(cols=False, tau=t, bias64=bias64, M64=A64, force=force, x64=fr.solve64(A64, force))   # A64 sets metric and residual
        c["e_qdd"], c["e_res"] = figures(fr.chol_solve(A32, force32, f32), c)
        out[name] = c
    c = dict(cols=True, tau=rhs, M64=A64, force=rhs.astype(np.float64), rhs=rhs,
             x64=fr.solve64(A64, rhs.astype(np.float64).transpose(0, 2, 1)).transpose(0, 2, 1))
    c["e_qdd"], c["e_res"] = figures(fr.chol_solve(A32, rhs.transpose(0, 2, 1), f32).transpose(0, 2, 1), c)
    out["msolve"] = c
    return out


def check(x, c, what):
    assert not np.isnan(x).any(), f"{what}: an element was not written"
    E, R = figures(x, c)
    print(f"{what}: E_qdd = {E:.3g} (fp32 reference {c['e_qdd']:.3g}, bound {FACTOR * c['e_qdd']:.3g}), "
          f"E_res = {R:.3g} (fp32 reference {c['e_res']:.3g}, bound {FACTOR * c['e_res']:.3g})")
    assert E <= FACTOR * c["e_qdd"] and R <= FACTOR * c["e_res"], what


# ------------------------------------------------------------------------------------------------- CPU
def test_abi_exports_and_null_handle(lib):
    for name in ("dexsim_forward_dynamics", "dexsim_mass_solve"):
        assert name in _abi.EXPORTED_SYMBOLS
        assert hasattr(lib, name), f"libdexsim.so does not export {name}"
    assert lib.dexsim_forward_dynamics(None, None, 1, None, None, None, 1, None, None) == 1  # DEXSIM_ERR_ARG
    assert b"null handle" in lib.dexsim_last_error()
    assert lib.dexsim_mass_solve(None, None, 1, None, None, 1, 0, None, None) == 1
    assert b"null handle" in lib.dexsim_last_error()


def test_reference_roundoff():
    """The measurement the GPU tolerances rest on, and its cap.  Measured over these 300 poses (E_qdd / E_res): full 4.83e-05 /
    1.43e-05, free 4.18e-05 / 4.94e-06, nograv 4.89e-05 / 8.57e-06, msolve 9.60e-05 / 8.81e-06.  The GPU tests recompute the figures on
    their own 70 poses."""
    _reference_roundoff(None, None)


def test_reference_roundoff_generic_model():
    """The same measurement and cap on the model of tests/generic_model.py, with its armatures in the solve.  Measured (E_qdd /
    E_res): full 1.62e-05 / 4.86e-06, free 5.64e-06 / 8.21e-06, nograv 1.08e-05 / 3.73e-06, msolve 1.38e-05 / 4.93e-06."""
    _reference_roundoff("generic", True)


def _reference_roundoff(model, armature):
    sc, ms = _setup(1, model=model)
    q = fr.regular_poses(kr.HandKin(ms), 300, seed=3)
    arm = np.array(np.ctypeslib.as_array(ms.armature), dtype=np.float64) if armature else None
    r = references(sc, ms, q, ir.random_rates(300, seed=4)[0], seed=5, arm=arm)
    for name in CASES:
        print(f"reference roundoff over 300 poses, {name}: e_qdd = {r[name]['e_qdd']:.3g}, e_res = {r[name]['e_res']:.3g}")
        assert 0 < FACTOR * r[name]["e_qdd"] <= 1e-3 and 0 < FACTOR * r[name]["e_res"] <= 1e-3, name


def test_reference_solve_against_numpy():
    """The hand-written Cholesky in float64 against numpy.linalg.solve: 1e-9 in E_qdd (cond of the d-scaled M is about 2e3)."""
    sc, ms = _setup(1)
    q = fr.regular_poses(kr.HandKin(ms), 20, seed=7)
    M64, b64 = ir.mass_bias(kr.oracle_pair(sc, ms)[1], q, ir.random_rates(20, seed=8)[0])
    _, tau = fr.targets(M64, b64, 9)
    rhs = tau.astype(np.float64) - b64
    E = fr.err_qdd(fr.chol_solve(M64, rhs), fr.solve64(M64, rhs), M64)
    cols = np.random.default_rng(1).uniform(-1, 1, (20, NJ, 4))
    E2 = fr.err_qdd(fr.chol_solve(M64, cols), fr.solve64(M64, cols), M64)
    print(f"chol_solve against numpy.linalg.solve in float64: E_qdd = {E:.3g} (vector), {E2:.3g} (4 columns)")
    assert 0 <= E <= 1e-9 and 0 <= E2 <= 1e-9
    assert fr.chol_solve(M64, rhs, np.float32).dtype == np.float32


def _armature_case(seed):
    """test_inverse_dynamics.py::test_different_model's scaled model with armatures of the size of M's own diagonal."""
    sc, ms = _setup(N, model="scaled")
    hk = kr.HandKin(ms)
    arm = fr.set_armature(ms, kr.oracle_pair(sc, ms)[1], 0.5 * (hk.geom.lo + hk.geom.hi))
    q = fr.regular_poses(hk, N, seed)
    qd = ir.random_rates(N, seed + 10)[0]
    return sc, ms, q, qd, arm


def _generic_case(seed):
    """The model of tests/generic_model.py with its own armatures (0.5-2 e-4 per joint: the size of M's diagonal on the finger joints)."""
    sc, ms = _setup(N, model="generic", free_bodies=True)
    hk = kr.HandKin(ms)
    arm = np.array(np.ctypeslib.as_array(ms.armature), dtype=np.float64)
    return sc, ms, fr.regular_poses(hk, N, seed), ir.random_rates(N, seed + 10)[0], arm


def test_missing_terms_are_discriminated():
    """What a kernel that dropped a term would return misses the bound by at least 100 x: the bias force (solve(M64, tau)), the
    gravity force (gravity off in place of on), and the armature on the armature test's model."""
    sc, ms = _setup(1)
    q = kr.HandKin(ms).random_poses(N, seed=21)
    r = references(sc, ms, q, ir.random_rates(N, seed=31)[0], seed=41)
    c = r["full"]
    tau = c["tau"].astype(np.float64)
    for what, x in (("without the bias force", fr.solve64(r["M64"], tau)), ("without gravity", fr.solve64(r["M64"], tau - r["c64"]))):
        miss = fr.err_qdd(x, c["x64"], r["M64"])
        print(f"fp64 solution {what}: E_qdd = {miss:.3g}, the bound is {FACTOR * c['e_qdd']:.3g}")
        assert miss >= 100 * FACTOR * c["e_qdd"]
    sc, ms, q, qd, arm = _armature_case(22)
    assert 1e-6 < arm[6:].min() and arm[6:].max() < 1e-3
    print(f"armatures: base {arm[:6].min():.3g} .. {arm[:6].max():.3g}, fingers {arm[6:].min():.3g} .. {arm[6:].max():.3g}")
    on, off = references(sc, ms, q, qd, seed=42, arm=arm), references(sc, ms, q, qd, seed=42)
    for name in CASES:
        miss = figures(off[name]["x64"], on[name])[0]
        print(f"armature left out, {name}: E_qdd = {miss:.3g}, the bound is {FACTOR * on[name]['e_qdd']:.3g}")
        assert miss >= 100 * FACTOR * on[name]["e_qdd"]
        miss = figures(on[name]["x64"], off[name])[0]                                   # and the flag set where it must not be
        assert miss >= 100 * FACTOR * off[name]["e_qdd"]


_stub_core = stub_core(dict(
    forward_dynamics=lambda out, tau=None, env_ids=None, q=None, qd=None, gravity=True, armature=False:
        ("fd", tuple(out.shape), tau is not None, q is not None, qd is not None, gravity, armature),
    mass_solve=lambda out, rhs, env_ids=None, q=None, armature=False: ("ms", tuple(out.shape), tuple(rhs.shape), q is not None, armature)))


def test_env_argument_validation():
    import torch
    from dexrobot_isaac_amd import make_env
    from oracle.py_backend import OracleCore
    env = make_env("BaseTask", 3, "cpu", "cpu", 0, _core_factory=_stub_core)
    z = lambda *s: torch.zeros(*s)
    fd, ms = env.get_forward_dynamics, env.solve_mass_matrix
    with pytest.raises(ValueError, match="q and qd"):
        fd(q=z(4, NJ))                                                          # q without qd
    with pytest.raises(ValueError, match="q and qd"):
        fd(qd=z(3, NJ))
    with pytest.raises(ValueError, match="shape"):
        fd(q=z(4, NJ), qd=z(5, NJ))
    with pytest.raises(ValueError, match="shape"):
        fd(q=z(4, NJ - 1), qd=z(4, NJ - 1))
    with pytest.raises(ValueError, match="out"):
        fd(out=z(4, NJ))
    with pytest.raises(ValueError, match="shape"):
        fd(tau=z(4, NJ))                                                        # three envs
    with pytest.raises(ValueError, match="shape"):
        fd(tau=z(3, NJ), env_ids=[0, 2])                                        # tau goes with the output rows
    with pytest.raises(ValueError, match="shape"):
        ms(z(4, NJ))
    with pytest.raises(ValueError, match="shape"):
        ms(z(3, NJ), env_ids=[0, 2])                                            # rhs goes with the output rows
    with pytest.raises(ValueError, match="shape"):
        ms(z(3, NJ), q=z(4, NJ))
    with pytest.raises(ValueError, match="shape"):
        ms(z(3, 2, NJ - 1))
    with pytest.raises(ValueError, match="shape"):
        ms(z(3, 2, 2, NJ))                                                      # two or three dimensions
    with pytest.raises(ValueError, match="shape"):
        ms(z(3 * NJ))
    with pytest.raises(ValueError, match="shape"):
        ms(z(3, 33, NJ))                                                        # nrhs <= 32
    with pytest.raises(ValueError, match="shape"):
        ms(z(3, 0, NJ))
    with pytest.raises(ValueError, match="out"):
        ms(z(3, 2, NJ), out=z(3, NJ))
    with pytest.raises(ValueError, match="out"):
        ms(z(3, NJ), out=z(3, 1, NJ))
    assert not env._core.calls                                                  # nothing reached the core
    assert fd(tau=z(2, NJ), env_ids=[2, 0], gravity=False).shape == (2, NJ)
    assert env._core.calls[-1] == ("fd", (2, NJ), True, False, False, False, False)
    assert fd(q=z(5, NJ), qd=z(5, NJ), armature=True).shape == (5, NJ)
    assert env._core.calls[-1] == ("fd", (5, NJ), False, True, True, True, True)
    assert ms(z(3, NJ)).shape == (3, NJ)
    assert env._core.calls[-1] == ("ms", (3, 1, NJ), (3, 1, NJ), False, False)
    assert ms(z(2, 32, NJ), env_ids=[1, 1], armature=True).shape == (2, 32, NJ)
    assert env._core.calls[-1] == ("ms", (2, 32, NJ), (2, 32, NJ), False, True)
    r = z(4, 5, NJ)
    assert ms(r, q=z(4, NJ), out=r) is r                                        # in place
    assert env._core.calls[-1] == ("ms", (4, 5, NJ), (4, 5, NJ), True, False)
    plain = make_env("BaseTask", 2, "cpu", "cpu", 0, _core_factory=OracleCore)  # the CPU stand-in has no such calls
    with pytest.raises(NotImplementedError):
        plain.get_forward_dynamics()
    with pytest.raises(NotImplementedError):
        plain.solve_mass_matrix(z(2, NJ))


# ------------------------------------------------------------------------------------------------- GPU helpers
def gpu_fd(core, k, tau=None, env_ids=None, q=None, qd=None, gravity=True, armature=False):
    full, out = _guarded(k, NJ)
    core.forward_dynamics(out, tau=_dev(tau), env_ids=env_ids, q=_dev(q), qd=_dev(qd), gravity=gravity, armature=armature)
    _guards_ok(full)
    return out.cpu().numpy()


def gpu_ms(core, k, rhs, env_ids=None, q=None, armature=False, in_place=False):
    rhs = np.asarray(rhs, dtype=np.float32)
    full, out = _guarded(k, rhs.shape[1], NJ)
    if in_place:
        out.copy_(_dev(rhs))
    core.mass_solve(out, out if in_place else _dev(rhs), env_ids=env_ids, q=_dev(q), armature=armature)
    _guards_ok(full)
    return out.cpu().numpy()


def gpu_id(core, k, qdd, q=None, qd=None):
    full, out = _guarded(k, NJ)
    core.inverse_dynamics(out, qdd=_dev(qdd), q=_dev(q), qd=_dev(qd), gravity=True)
    _guards_ok(full)
    return out.cpu().numpy()


def gpu_all(core, c, k, armature=False, **rows):
    """The four cases of `references` on the device."""
    return dict(full=gpu_fd(core, k, tau=c["full"]["tau"], armature=armature, **rows), free=gpu_fd(core, k, armature=armature, **rows),
                nograv=gpu_fd(core, k, tau=c["nograv"]["tau"], gravity=False, armature=armature, **rows),
                msolve=gpu_ms(core, k, c["msolve"]["rhs"], armature=armature, **{a: v for a, v in rows.items() if a != "qd"}))


def check_all(got, c, what):
    for name in CASES:
        check(got[name], c[name], f"{what}, {name}")


def _core_at(sc, ms, q, qd):
    from dexrobot_isaac_amd.core import DexSimCore
    core = DexSimCore(sc, ms, "cuda:0")
    core.reset()
    pose_core(core, q, qd=qd)
    assert (core.field("qd").t().cpu().numpy() == qd).all()
    return core


@pytest.fixture(scope="module")
def posed():
    sc, ms = _setup(N)
    q = kr.HandKin(ms).random_poses(N, seed=21)
    qd = ir.random_rates(N, seed=31)[0]
    c = references(sc, ms, q, qd, seed=41)
    c["core"] = _core_at(sc, ms, q, qd)
    c["got"] = gpu_all(c["core"], c, N)
    return c


# ------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_accuracy_against_fp64(posed):
    c = posed
    check_all(c["got"], c, "default model")
    still = gpu_fd(c["core"], N, q=c["q"], qd=np.zeros_like(c["qd"]), gravity=False)
    assert (still == 0).all()                                                  # no force, nothing moves: exact zeros


@pytest.mark.gpu
def test_consistency_on_the_device(posed):
    """Two round trips on the device, bounds in E_tau's per-joint scaling d_j = sqrt(M64_jj), S(t) = the pose's max_j |t|_j / d_j.

    dexsim_inverse_dynamics(q, qd, qdd_dev) against tau: the inverse dynamics is within 4 e_id of M64 qdd_dev + b64 (its own bound,
    test_inverse_dynamics's e_full recomputed at accelerations of this size), and that force is within 4 e_res of tau (this suite's
    residual bound), both relative to S(tau): the two differ by at most 4 (e_id + e_res) S(tau).

    M_dev @ X for X = the mass solve of the 26 unit columns against the identity: column r of M64 X is within 4 e_res S(e_r) =
    4 e_res / d_r of e_r (the residual bound for that column; e_res is the fp32 reference's figure for the SAME unit columns), and
    |M_dev - M64|_ji <= 4 e_M d_j d_i (test_kindyn's bound) moves (M X)_jr / d_j by at most 4 e_M sum_i d_i |X_ir|: the sum of the two."""
    c = posed
    core, M64 = c["core"], c["M64"]
    d = np.sqrt(np.einsum("nii->ni", M64))
    back = gpu_id(core, N, c["got"]["full"])
    E = ir.err_tau(back, c["full"]["tau"].astype(np.float64), M64)
    bound = FACTOR * (c["e_id"] + c["full"]["e_res"])
    print(f"inverse_dynamics(forward_dynamics(tau)) against tau: E_tau = {E:.3g}, bound {bound:.3g}")
    assert E <= bound
    eye = np.broadcast_to(np.eye(NJ, dtype=np.float32), (N, NJ, NJ)).copy()
    X = gpu_ms(core, N, eye)                                                   # X[n, r, :] = M^-1 e_r
    ref = dict(cols=True, M64=M64, force=eye.astype(np.float64), x64=fr.solve64(M64, eye.astype(np.float64)).transpose(0, 2, 1))
    ref["e_qdd"], ref["e_res"] = figures(fr.chol_solve(c["M32"], eye, np.float32).transpose(0, 2, 1), ref)
    check(X, ref, "M^-1 from 26 unit columns")
    fm, Md = _guarded(N, NJ, NJ)
    core.mass_matrix(mass=Md)
    _guards_ok(fm)
    prod = np.einsum("nji,nri->nrj", Md.cpu().numpy().astype(np.float64), X.astype(np.float64))   # [n, r, j] = (M_dev x_r)_j
    err = (np.abs(prod - eye) / d[:, None, :]).max(2)                                              # per pose and column
    bound = FACTOR * (ref["e_res"] / d + c["e_M"] * (np.abs(X) * d[:, None, :]).sum(2))
    print(f"M_dev @ M^-1 against the identity: worst error / bound = {(err / bound).max():.3g}")
    assert (err <= bound).all()


@pytest.mark.gpu
def test_armature_and_different_model():
    """The scaled model with general finger inertias and armatures of the size of M's diagonal: flag on against
    solve(M64 + diag(a), .), flag off against solve(M64, .) -- test_missing_terms_are_discriminated shows that either one misses the
    other's bound by 100 x."""
    sc, ms, q, qd, arm = _armature_case(22)
    core = _core_at(sc, ms, q, qd)
    on, off = references(sc, ms, q, qd, seed=42, arm=arm), references(sc, ms, q, qd, seed=42)
    check_all(gpu_all(core, on, N, armature=True), on, "scaled model, armature")
    check_all(gpu_all(core, off, N), off, "scaled model, no armature")
    core.close()


@pytest.mark.gpu
def test_structure_free_model():
    """The model of tests/generic_model.py, which has none of the default model's exact zeros, ones and repeated numbers: every
    case with and without its armatures, the bounds recomputed from the float32 reference on these rows of this model."""
    sc, ms, q, qd, arm = _generic_case(23)
    core = _core_at(sc, ms, q, qd)
    on, off = references(sc, ms, q, qd, seed=43, arm=arm), references(sc, ms, q, qd, seed=43)
    check_all(gpu_all(core, on, N, armature=True), on, "generic model, armature")
    check_all(gpu_all(core, off, N), off, "generic model, no armature")
    core.close()


@pytest.mark.gpu
def test_addressing(posed):
    import torch
    c = posed
    core, q, qd, got = c["core"], c["q"], c["qd"], c["got"]
    tau, tau0, rhs = c["full"]["tau"], c["nograv"]["tau"], c["msolve"]["rhs"]
    ids = [69, 0, 64, 3, 63]                                                   # out of order; tau / rhs ride with the output rows
    assert (bits(gpu_fd(core, len(ids), env_ids=ids, tau=tau[ids])) == bits(got["full"][ids])).all()
    assert (bits(gpu_fd(core, len(ids), env_ids=ids)) == bits(got["free"][ids])).all()
    assert (bits(gpu_fd(core, len(ids), env_ids=ids, tau=tau0[ids], gravity=False)) == bits(got["nograv"][ids])).all()
    assert (bits(gpu_ms(core, len(ids), rhs[ids], env_ids=ids)) == bits(got["msolve"][ids])).all()
    assert (bits(gpu_fd(core, 1, env_ids=[37], tau=tau[[37]])) == bits(got["full"][[37]])).all()       # k = 1
    assert (bits(gpu_ms(core, 1, rhs[[37]], env_ids=[37])) == bits(got["msolve"][[37]])).all()
    # overrides, k = 130 (three workgroups): rows copied from env state are the state path's bits, the rest meet the reference
    n_new = 130 - N
    qn = fr.regular_poses(c["hk"], n_new, seed=23)
    vn = ir.random_rates(n_new, seed=24)[0]
    cn = references(c["sc"], core.model, qn, vn, seed=25)
    src = np.concatenate([np.arange(40), np.full(n_new, -1), np.arange(40, N)])
    st = src >= 0
    cat = lambda old, new: np.concatenate([old[:40], new, old[40:]])
    both = {name: dict(tau=None if name == "free" else cat(c[name]["tau"], cn[name]["tau"])) for name in CASES}
    both["msolve"]["rhs"] = both["msolve"]["tau"]
    over = gpu_all(core, both, 130, q=cat(q, qn), qd=cat(qd, vn), env_ids=[-1])                        # env_ids is ignored with overrides
    for name in CASES:
        assert (bits(over[name][st]) == bits(got[name][src[st]])).all(), name
    check_all({name: over[name][~st] for name in CASES}, cn, "overrides")
    # ids outside [0, N) leave their rows as they are
    bad = [5, -1, N, 69]
    xb, mb = gpu_fd(core, 4, env_ids=bad, tau=tau[[5, 0, 0, 69]]), gpu_ms(core, 4, rhs[[5, 0, 0, 69]], env_ids=bad)
    assert np.isnan(xb[1:3]).all() and np.isnan(mb[1:3]).all()
    assert (bits(xb[[0, 3]]) == bits(got["full"][[5, 69]])).all() and (bits(mb[[0, 3]]) == bits(got["msolve"][[5, 69]])).all()
    # a column's bits do not depend on nrhs or on its position; in place
    wide = np.random.default_rng(51).uniform(-1, 1, (N, 32, NJ)).astype(np.float32)
    wide[:, 7], wide[:, 31], wide[:, 4] = rhs[:, 0], rhs[:, 1], rhs[:, 2]
    x32 = gpu_ms(core, N, wide)
    assert not np.isnan(x32).any()
    assert (bits(x32[:, [7, 31, 4]]) == bits(got["msolve"])).all()
    assert (bits(gpu_ms(core, N, rhs[:, [1]])) == bits(got["msolve"][:, [1]])).all()
    assert (bits(gpu_ms(core, N, wide[:, :6])[:, 4]) == bits(got["msolve"][:, 2])).all()
    assert (bits(gpu_ms(core, N, wide, in_place=True)) == bits(x32)).all()
    assert (bits(gpu_ms(core, N, rhs, in_place=True)) == bits(got["msolve"])).all()
    # forward dynamics at qd = 0 without flags is the mass solve of tau: the same bits
    rest = gpu_fd(core, N, tau=rhs[:, 0], q=q, qd=np.zeros_like(qd), gravity=False)
    assert (bits(rest) == bits(got["msolve"][:, 0])).all()
    # argument errors come back as DEXSIM_ERR_ARG with their message, before any launch
    lib, h = core.lib, core.h
    out = torch.full((130, 3, NJ), float("nan"), device=core.device)
    po, po2 = C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr() + 2)
    keep = [_dev(a) for a in (cat(q, qn), cat(qd, vn), both["msolve"]["rhs"])]
    pq, pv, pr = (C.c_void_p(t.data_ptr()) for t in keep)

    def refused(rc, text):
        assert rc == 1 and text in lib.dexsim_last_error(), (rc, lib.dexsim_last_error())
    refused(lib.dexsim_forward_dynamics(h, None, 0, None, None, None, 1, po, None), b"k must be positive")
    refused(lib.dexsim_forward_dynamics(h, None, N - 1, None, None, None, 1, po, None), b"k == num_envs")
    refused(lib.dexsim_forward_dynamics(h, None, 130, pq, None, None, 1, po, None), b"q and qd")
    refused(lib.dexsim_forward_dynamics(h, None, N, None, pv, None, 1, po, None), b"q and qd")
    refused(lib.dexsim_forward_dynamics(h, None, N, None, None, None, 4, po, None), b"flag")
    refused(lib.dexsim_forward_dynamics(h, None, N, None, None, None, 3, None, None), b"qdd")
    refused(lib.dexsim_forward_dynamics(h, None, N, None, None, None, 3, po2, None), b"qdd")
    refused(lib.dexsim_mass_solve(h, None, 0, None, pr, 3, 0, po, None), b"k must be positive")
    refused(lib.dexsim_mass_solve(h, None, N - 1, None, pr, 3, 0, po, None), b"k == num_envs")
    refused(lib.dexsim_mass_solve(h, None, N, None, pr, 3, 1, po, None), b"flag")                     # DEXSIM_FD_GRAVITY
    refused(lib.dexsim_mass_solve(h, None, N, None, pr, 3, 4, po, None), b"flag")
    refused(lib.dexsim_mass_solve(h, None, N, None, pr, 0, 0, po, None), b"nrhs")
    refused(lib.dexsim_mass_solve(h, None, N, None, pr, 33, 0, po, None), b"nrhs")
    refused(lib.dexsim_mass_solve(h, None, N, None, None, 3, 0, po, None), b"rhs")
    refused(lib.dexsim_mass_solve(h, None, N, None, pr, 3, 0, None, None), b"out")
    refused(lib.dexsim_mass_solve(h, None, N, None, pr, 3, 2, po2, None), b"out")
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                                              # nothing was launched


@pytest.mark.gpu
def test_purity():
    import torch
    rng = np.random.default_rng(41)
    tau, rhs = rng.uniform(-1, 1, (N, NJ)).astype(np.float32), rng.uniform(-1, 1, (N, 5, NJ)).astype(np.float32)
    rnd = lambda *s: torch.rand(*s, device="cuda:0")

    def between(core):
        gpu_fd(core, 3, env_ids=[69, 1, 64], gravity=False, armature=True)
        gpu_ms(core, 3, rhs[:3], env_ids=[69, 1, 64], armature=True)
        gpu_fd(core, 100, q=rnd(100, NJ), qd=rnd(100, NJ), tau=rnd(100, NJ))
        gpu_ms(core, 100, rnd(100, 32, NJ).cpu().numpy(), q=rnd(100, NJ), in_place=True)
    x1, m1 = purity_frame(lambda core: [gpu_fd(core, N, tau=tau), gpu_ms(core, N, rhs)], between, n=N)
    assert not np.isnan(x1).any() and not np.isnan(m1).any() and np.abs(x1).max() > 0


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
    tau = env.get_inverse_dynamics((20 * torch.rand(N, NJ, generator=g) - 10).cuda())          # forces of a sensible size
    assert env.get_forward_dynamics(tau).shape == (N, NJ)                      # allocated by the call
    full, out = _guarded(N, NJ)
    qdd = env.get_forward_dynamics(tau, out=out)
    _guards_ok(full)
    assert qdd is out and not torch.isnan(qdd).any()
    free = env.get_forward_dynamics()
    assert free.shape == (N, NJ) and not torch.equal(free, env.get_forward_dynamics(gravity=False))
    assert torch.equal(env.get_forward_dynamics(tau[[3, 1]], env_ids=[3, 1]).view(torch.int32), qdd[[3, 1]].view(torch.int32))
    with pytest.raises(ValueError):
        env.get_forward_dynamics(q=env.dof_pos.clone())
    q0, v0 = env.dof_pos.clone(), env.dof_vel.clone()                          # the overrides at the current state: the state path's bits
    assert torch.equal(env.get_forward_dynamics(tau, q=q0, qd=v0).view(torch.int32), qdd.view(torch.int32))
    back = env.get_inverse_dynamics(qdd)                                       # the round trip
    assert bool(torch.isfinite(back).all())
    M64 = env.get_mass_matrix().double().cpu().numpy()
    E = ir.err_tau(back.cpu().numpy(), tau.double().cpu().numpy(), M64)
    print(f"get_inverse_dynamics(get_forward_dynamics(tau)) against tau: E_tau = {E:.3g}")
    assert E <= 1e-3                                                           # test_reference_roundoff's cap
    rhs = (2 * torch.rand(N, 4, NJ, generator=g) - 1).cuda()
    assert env.solve_mass_matrix(rhs).shape == (N, 4, NJ) and env.solve_mass_matrix(rhs[:, 0]).shape == (N, NJ)
    full, out = _guarded(N, 4, NJ)
    x = env.solve_mass_matrix(rhs, out=out)
    _guards_ok(full)
    assert x is out and not torch.isnan(x).any()
    assert torch.equal(env.solve_mass_matrix(rhs[:, 2]).view(torch.int32), x[:, 2].view(torch.int32))
    assert torch.equal(env.solve_mass_matrix(rhs[[5, 69]], env_ids=[5, 69]).view(torch.int32), x[[5, 69]].view(torch.int32))
    assert torch.equal(env.solve_mass_matrix(rhs, q=q0).view(torch.int32), x.view(torch.int32))
    # Lambda^-1 = J M^-1 J^T of one fingertip's three linear rows: symmetric to roundoff and positive definite
    J = env.get_jacobian(bodies=["r_f_link1_tip"])[:, 0, 0:3, :].contiguous()                     # (N, 3, 26)
    Li = torch.einsum("nij,nkj->nik", J, env.solve_mass_matrix(J)).double()
    assert Li.shape == (N, 3, 3)
    scale = Li.diagonal(dim1=1, dim2=2).abs().amax(1)[:, None, None]
    asym = float(((Li - Li.transpose(1, 2)).abs() / scale).max())
    print(f"Lambda^-1 of a fingertip: asymmetry {asym:.3g} of its largest diagonal entry")
    assert asym <= 2e-3                                                        # two entries, each within the suite's 1e-3 roundoff cap
    assert float(torch.linalg.eigvalsh(0.5 * (Li + Li.transpose(1, 2))).min()) > 0
    env.close()
