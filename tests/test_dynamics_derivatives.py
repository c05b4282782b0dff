"""Derivatives of the inverse and the forward dynamics on the device (dexsim_inverse_dynamics_derivatives,
dexsim_forward_dynamics_derivatives) against tests/dynderiv_ref.py: the analytic float64 derivative of the Newton-Euler recursion
(validated here against central differences of the fp64 CPU oracle), and -solve(M64 [+ diag a], .) of it at qdd64 for the forward
route.

Inputs: poses from fwddyn_ref.regular_poses with |cos q4| >= 0.3 (the full joint range without the 17 degrees around the base's
gimbal lock, where M is singular and d qdd is unbounded: test_reference_roundoff says why not the default 0.1), qd and qdd from invdyn_ref.random_rates (+-3, +-10), tau from fwddyn_ref.targets, the second
model from query_rig.scaled_model / fwddyn_ref.set_armature, the third from tests/generic_model.py.

Metrics (dynderiv_ref.err_dtau, err_dqdd), with d_r = sqrt(M64_rr) and D[r, c] = d_r / d_c the Jacobian: E_dtau is per pose
max_rc |D - D64|_rc / d_r over max_rc |D64|_rc / d_r, E_dqdd the same with |.|_rc d_r; the max over poses.  A pose counts as a whole.

Tolerances: FACTOR = 4 x the same figure of the float32 reference on the SAME poses -- dynderiv_ref.id_derivatives evaluated in
float32, and for the forward route fwddyn_ref.chol_solve in float32 on the fp32 oracle's M32 and b32 -- recomputed by every test;
test_kindyn.py gives the factor's reasons.  test_reference_roundoff caps 4 x every figure at 1e-2 on 300 poses.

Every GPU test uses N = 70: two workgroups, six live lanes in the second; every device output sits between two guard rows that
must come back untouched.  Device arrays are derivative-major, out[i, c, r]; `jac` below turns them into Jacobians.

Measured on one MI355X (profiles/dynamics_derivatives/README.md has the full list), device against fp32 reference, d/dq and d/dqd:
inverse full 8.64e-07 / 1.41e-06 and 1.17e-06 / 2.78e-06, flags = 0 9.96e-07 / 1.82e-06, qdd NULL 1.22e-06 / 2.56e-06; forward full
1.25e-05 / 1.71e-04 and 1.25e-05 / 1.92e-04, free 2.95e-04 / 1.57e-03; scaled model with armature 1.09e-06 / 5.17e-06 and 8.30e-07 /
3.43e-06, without 8.69e-06 / 3.45e-05 and 9.89e-06 / 3.88e-05.  Consistency: the qd identity 1.40e-05 (reference 1.40e-05), the
Hessian's asymmetry 1.13e-07 (reference 7.92e-07).  Public surface: D @ dq against the change of get_inverse_dynamics 0.0261 of
the first-order change, the fp64 second-order remainder 0.0261, bound 0.104.
"""
import ctypes as C

import numpy as np
import pytest

from dexrobot_isaac_amd import _abi
from tests import dynderiv_ref as dd
from tests import fwddyn_ref as fr
from tests import invdyn_ref as ir
from tests import kindyn_ref as kr
from tests.query_rig import (bits, dev as _dev, guarded as _guarded, guards_ok as _guards_ok, load_lib, pose_core, purity_frame,
                             setup as _setup, stub_core)

N = 70
NJ = _abi.NJ
FACTOR = 4
ID_CASES = ("full", "noflags", "bias")        # gravity and qdd | flags = 0 | qdd NULL
f32 = np.float32
MIN_COS = 0.3


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def poses(hk, n, seed):
    """fwddyn_ref.regular_poses with |cos q4| >= MIN_COS."""
    return fr.regular_poses(hk, n, seed, min_cos=MIN_COS)


def jac(a):
    """Device layout (k, c, r) -> Jacobian (k, r, c)."""
    return np.asarray(a).transpose(0, 2, 1)


# ------------------------------------------------------------------------------------------------- references
def references(sc, ms, q, qd, seed, arm=None, forward=("full", "free")):
    """Every reference of the poses (q, qd), computed once.  Inverse cases ID_CASES: the fp64 Jacobians D64 = (dq, dqd) and the
    float32 reference's own figures e = (e_dq, e_dqd).  Forward cases `forward` (tau of fwddyn_ref.targets | tau NULL), with the
    armature `arm` (float64) in the solve if given: qdd64, X64 = (dqdd_dq, dqdd_dqd), e likewise, e_qdd for the acceleration."""
    o32, o64 = kr.oracle_pair(sc, ms)
    hk, links = kr.HandKin(ms), dd.Links(ms)
    grav = np.array(sc.gravity, dtype=np.float64)
    M64, b64 = ir.mass_bias(o64, q, qd)
    M32, b32 = ir.mass_bias(o32, q, qd)
    qdd = ir.random_rates(len(q), seed)[1]
    f64s, f32s = dd.frames(hk, q), dd.frames(hk, q, f32)
    ref = lambda a, g, dt, fs: dd.id_derivatives(hk, links, q, qd, a, g, dt, fs)
    out = dict(q=q, qd=qd, qdd=qdd, M64=M64, b64=b64, M32=M32, sc=sc, hk=hk, links=links, grav=grav, arm=arm)
    for name, (a, g) in dict(full=(qdd, grav), noflags=(qdd, None), bias=(None, grav)).items():
        t64, t32 = ref(a, g, np.float64, f64s), ref(a, g, f32, f32s)
        out[name] = dict(qdd=a, gravity=g is not None, tau64=t64[0], D64=t64[1:], D32=t32[1:],
                         e=(dd.err_dtau(t32[1], t64[1], M64), dd.err_dtau(t32[2], t64[2], M64)))
    A64 = M64 if arm is None else M64 + np.diag(arm)[None]
    A32 = (M32 if arm is None else M32 + np.diag(arm)[None]).astype(f32)
    _, tau = fr.targets(M64, b64, seed + 1)
    for name in forward:
        t = tau if name == "full" else None
        force64 = -b64 if t is None else t.astype(np.float64) - b64
        force32 = -b32.astype(f32) if t is None else t - b32.astype(f32)
        qdd64, qdd32 = fr.solve64(A64, force64), fr.chol_solve(A32, force32, f32)
        X64 = dd.fd_derivatives(A64, *ref(qdd64, grav, np.float64, f64s)[1:])
        X32 = dd.fd_derivatives(A32, *ref(qdd32, grav, f32, f32s)[1:], f32)
        out["fd_" + name] = dict(tau=t, qdd64=qdd64, X64=X64, e_qdd=fr.err_qdd(qdd32, qdd64, M64),
                                 e=(dd.err_dqdd(X32[0], X64[0], M64), dd.err_dqdd(X32[1], X64[1], M64)))
    return out


def check(got, want, e, M64, err, what):
    for g, w, ei, n in zip(got, want, e, ("d/dq", "d/dqd")):
        assert not np.isnan(g).any(), f"{what} {n}: an element was not written"
        E = err(jac(g), w, M64)
        print(f"{what} {n}: E = {E:.3g} (fp32 reference {ei:.3g}, bound {FACTOR * ei:.3g})")
        assert E <= FACTOR * ei, f"{what} {n}"


# ------------------------------------------------------------------------------------------------- CPU
def test_abi_exports_and_null_handle(lib):
    for name in ("dexsim_inverse_dynamics_derivatives", "dexsim_forward_dynamics_derivatives"):
        assert name in _abi.EXPORTED_SYMBOLS
        assert hasattr(lib, name), f"libdexsim.so does not export {name}"
    assert len(_abi.EXPORTED_SYMBOLS) == 50
    assert lib.dexsim_inverse_dynamics_derivatives(None, None, 1, None, None, None, 1, None, None, None) == 1  # DEXSIM_ERR_ARG
    assert b"null handle" in lib.dexsim_last_error()
    assert lib.dexsim_forward_dynamics_derivatives(None, None, 1, None, None, None, 1, None, None, None, None) == 1
    assert b"null handle" in lib.dexsim_last_error()


def test_reference_against_oracle_differences():
    """The analytic recursion in float64 against central differences of the fp64 oracle's tau = M qdd + b, h = 1e-4 in q and 1e-3
    in qd (differences at h and h / 10 agree to 2e-9 and 2e-10), bound 1e-7 in E_dtau; with gravity, and the zero-gravity oracle
    for flags = 0.  Measured on these 6 poses: 1.47e-08 / 1.82e-11 with gravity, 1.10e-08 / 7.4e-12 without; tau itself agrees
    with the oracle's to 6e-15.  (Over HandGeometry.fk, which normalises the model's float32 quaternions where the engine and the
    oracle do not, d/dqd was off by 1.3e-7: dynderiv_ref.frames.)"""
    _against_oracle_differences(None)


def test_reference_against_oracle_differences_generic_model():
    """The same on the model of tests/generic_model.py."""
    _against_oracle_differences("generic")


def _against_oracle_differences(model):
    from oracle.oracle import Oracle
    sc, ms = _setup(1, model=model)
    hk, links = kr.HandKin(ms), dd.Links(ms)
    q = poses(hk, 6, seed=3)
    qd, qdd = ir.random_rates(6, seed=4)
    for orc, grav in ((Oracle(sc, ms, f64=True), np.array(sc.gravity, dtype=np.float64)), (Oracle(ir.zero_gravity_config(1), ms, f64=True), None)):
        M64, _ = ir.mass_bias(orc, q, qd)
        tau, Dq, Dv = dd.id_derivatives(hk, links, q, qd, qdd, grav)
        tau_o = np.stack([dd.oracle_tau(orc, q[i], qd[i], qdd[i]) for i in range(6)])
        Cq, Cv = dd.central_differences(orc, q, qd, qdd, 1e-4, 1e-3)
        Eq, Ev, Et = dd.err_dtau(Dq, Cq, M64), dd.err_dtau(Dv, Cv, M64), ir.err_tau(tau, tau_o, M64)
        print(f"analytic against central differences ({'with' if grav is not None else 'no'} gravity): E_dtau = {Eq:.3g} (q), {Ev:.3g} (qd); tau {Et:.3g}")
        assert 0 < Eq <= 1e-7 and 0 < Ev <= 1e-7 and Et <= 1e-12
    assert dd.id_derivatives(hk, links, q, qd, qdd, None, f32)[1].dtype == f32


def test_reference_roundoff():
    """The measurement the GPU tolerances rest on, and its cap: 4 x every figure of the float32 reference stays below 1e-2.
    Measured over these 300 poses (d/dq, d/dqd): inverse full 2.43e-06 / 3.36e-06, noflags 3.16e-06 / 3.36e-06, bias 3.19e-06 /
    3.36e-06; forward full 2.10e-04 / 1.94e-04, free 1.86e-03 / 1.94e-04.  The GPU tests recompute the figures on their own 70
    poses.  With fwddyn_ref.regular_poses' default |cos q4| >= 0.1 the free acceleration's d/dq figure was 2.88e-03, 4 x that above
    the cap: d qdd grows with 1 / cos^2 q4, the inputs were wrong for this quantity, and every draw of this suite asks for
    |cos q4| >= MIN_COS = 0.3."""
    _reference_roundoff(None)


def test_reference_roundoff_generic_model():
    """The same measurement and cap on the model of tests/generic_model.py, its armatures in the forward route."""
    _reference_roundoff("generic")


def _reference_roundoff(model):
    sc, ms = _setup(1, model=model)
    q = poses(kr.HandKin(ms), 300, seed=3)
    arm = None if model is None else np.array(np.ctypeslib.as_array(ms.armature), dtype=np.float64)
    r = references(sc, ms, q, ir.random_rates(300, seed=4)[0], seed=5, arm=arm)
    for name in ID_CASES + ("fd_full", "fd_free"):
        print(f"reference roundoff over 300 poses, {name}: e = {r[name]['e'][0]:.3g} (d/dq), {r[name]['e'][1]:.3g} (d/dqd)")
        assert all(0 < FACTOR * e <= 1e-2 for e in r[name]["e"]), name


@pytest.fixture(scope="module")
def cpu_refs():
    sc, ms = _setup(1)
    q = poses(kr.HandKin(ms), N, seed=21)
    return references(sc, ms, q, ir.random_rates(N, seed=31)[0], seed=41)


def test_missing_terms_and_layout_are_discriminated(cpu_refs):
    """What a kernel that dropped a term, or wrote the Jacobian instead of its transpose, would return misses the bound on the
    GPU tests' own kind of inputs: the fp64 result without gravity, without (dM/dq) qdd (qdd NULL) and without the velocity terms
    (qd = 0) against the full one, and every matrix against its transpose."""
    r = cpu_refs
    full = r["full"]
    M64 = r["M64"]
    still = dd.id_derivatives(r["hk"], r["links"], r["q"], np.zeros_like(r["qd"]), r["qdd"], r["grav"])[1:]
    for what, other in (("without gravity", r["noflags"]["D64"]), ("without (dM/dq) qdd", r["bias"]["D64"]), ("at qd = 0", still)):
        for i, n in enumerate(("d/dq", "d/dqd")):
            if what != "at qd = 0" and i == 1:
                continue                                                       # gravity and M qdd do not depend on qd
            miss = dd.err_dtau(other[i], full["D64"][i], M64)
            print(f"fp64 result {what}, {n}: E_dtau = {miss:.3g}, the bound is {FACTOR * full['e'][i]:.3g}")
            assert miss > 10 * FACTOR * full["e"][i]
    for name, err in (("full", dd.err_dtau), ("noflags", dd.err_dtau), ("bias", dd.err_dtau), ("fd_full", dd.err_dqdd), ("fd_free", dd.err_dqdd)):
        D = r[name]["D64"] if name in ID_CASES else r[name]["X64"]
        for i, n in enumerate(("d/dq", "d/dqd")):
            miss = err(D[i].transpose(0, 2, 1), D[i], M64)
            print(f"{name} {n} transposed: E = {miss:.3g}, the bound is {FACTOR * r[name]['e'][i]:.3g}")
            assert miss > 10 * FACTOR * r[name]["e"][i]


_stub_core = stub_core(dict(
    inverse_dynamics_derivatives=lambda dq, dqd, qdd=None, env_ids=None, q=None, qd=None, gravity=True:
        ("idd", tuple(dq.shape), tuple(dqd.shape), qdd is not None, q is not None, qd is not None, gravity),
    forward_dynamics_derivatives=lambda qdd, dq, dqd, tau=None, env_ids=None, q=None, qd=None, gravity=True, armature=False:
        ("fdd", tuple(qdd.shape), tuple(dq.shape), tuple(dqd.shape), tau is not None, q is not None, qd is not None, gravity, armature)))


def test_env_argument_validation():
    import torch
    from dexrobot_isaac_amd import make_env
    from oracle.py_backend import OracleCore
    env = make_env("BaseTask", 3, "cpu", "cpu", 0, _core_factory=_stub_core)
    z = lambda *s: torch.zeros(*s)
    for fn, arg in ((env.get_inverse_dynamics_derivatives, "qdd"), (env.get_forward_dynamics_derivatives, "tau")):
        with pytest.raises(ValueError, match="q and qd"):
            fn(q=z(4, NJ))                                                      # q without qd
        with pytest.raises(ValueError, match="q and qd"):
            fn(qd=z(3, NJ))
        with pytest.raises(ValueError, match="shape"):
            fn(q=z(4, NJ), qd=z(5, NJ))
        with pytest.raises(ValueError, match="shape"):
            fn(q=z(4, NJ - 1), qd=z(4, NJ - 1))
        with pytest.raises(ValueError, match="shape"):
            fn(z(4, NJ))                                                        # three envs
        with pytest.raises(ValueError, match="shape"):
            fn(z(3, NJ), env_ids=[0, 2])                                        # qdd / tau go with the output rows
        with pytest.raises(ValueError, match="out"):
            fn(out=z(3, NJ, NJ))                                                # not a tuple
        with pytest.raises(ValueError, match="out"):
            fn(out=(z(3, NJ, NJ),))
    with pytest.raises(ValueError, match="out"):
        env.get_inverse_dynamics_derivatives(out=(z(3, NJ, NJ), z(3, NJ)))
    with pytest.raises(ValueError, match="out"):
        env.get_forward_dynamics_derivatives(out=(z(3, NJ, NJ), z(3, NJ, NJ), z(3, NJ, NJ)))
    assert not env._core.calls                                                  # nothing reached the core
    dq, dqd = env.get_inverse_dynamics_derivatives(z(2, NJ), env_ids=[2, 0], gravity=False)
    assert dq.shape == (2, NJ, NJ) and dqd.shape == (2, NJ, NJ)
    assert env._core.calls[-1] == ("idd", (2, NJ, NJ), (2, NJ, NJ), True, False, False, False)
    o = (z(5, NJ, NJ), z(5, NJ, NJ))
    dq, dqd = env.get_inverse_dynamics_derivatives(q=z(5, NJ), qd=z(5, NJ), out=o)
    assert dq.data_ptr() == o[0].data_ptr() and dqd.data_ptr() == o[1].data_ptr()      # transposed views of the outputs given
    assert env._core.calls[-1] == ("idd", (5, NJ, NJ), (5, NJ, NJ), False, True, True, True)
    qdd, dq, dqd = env.get_forward_dynamics_derivatives(armature=True)
    assert qdd.shape == (3, NJ) and dq.shape == (3, NJ, NJ) and dqd.shape == (3, NJ, NJ)
    assert env._core.calls[-1] == ("fdd", (3, NJ), (3, NJ, NJ), (3, NJ, NJ), False, False, False, True, True)
    plain = make_env("BaseTask", 2, "cpu", "cpu", 0, _core_factory=OracleCore)  # the CPU stand-in has no such calls
    with pytest.raises(NotImplementedError):
        plain.get_inverse_dynamics_derivatives()
    with pytest.raises(NotImplementedError):
        plain.get_forward_dynamics_derivatives()


# ------------------------------------------------------------------------------------------------- GPU helpers
def gpu_idd(core, k, qdd=None, env_ids=None, q=None, qd=None, gravity=True, which=(True, True)):
    """(dtau_dq, dtau_dqd) in the device's layout; an output left out (`which`) comes back as None."""
    bufs = [_guarded(k, NJ, NJ) if w else (None, None) for w in which]
    core.inverse_dynamics_derivatives(bufs[0][1], bufs[1][1], qdd=_dev(qdd), env_ids=env_ids, q=_dev(q), qd=_dev(qd), gravity=gravity)
    for full, _ in bufs:
        if full is not None:
            _guards_ok(full)
    return tuple(None if o is None else o.cpu().numpy() for _, o in bufs)


def gpu_fdd(core, k, tau=None, env_ids=None, q=None, qd=None, gravity=True, armature=False, which=(True, True)):
    """(qdd, dqdd_dq, dqdd_dqd) in the device's layout."""
    fa, qdd = _guarded(k, NJ)
    bufs = [_guarded(k, NJ, NJ) if w else (None, None) for w in which]
    core.forward_dynamics_derivatives(qdd, bufs[0][1], bufs[1][1], tau=_dev(tau), env_ids=env_ids, q=_dev(q), qd=_dev(qd), gravity=gravity,
                                      armature=armature)
    for full in [fa] + [b[0] for b in bufs]:
        if full is not None:
            _guards_ok(full)
    return (qdd.cpu().numpy(),) + tuple(None if o is None else o.cpu().numpy() for _, o in bufs)


def gpu_call(core, fn, k, *a, **kw):
    full, out = _guarded(k, *a)
    fn(out, **{n: _dev(v) if isinstance(v, np.ndarray) else v for n, v in kw.items()})
    _guards_ok(full)
    return out.cpu().numpy()


def gpu_all(core, c, k, armature=False, **rows):
    """Every case of `references` on the device."""
    got = {name: gpu_idd(core, k, qdd=c[name]["qdd"], gravity=c[name]["gravity"], **rows) for name in ID_CASES if name in c}
    for name in ("fd_full", "fd_free"):
        if name in c:
            got[name] = gpu_fdd(core, k, tau=c[name]["tau"], armature=armature, **rows)
    return got


def check_all(got, c, what):
    for name in got:
        if name in ID_CASES:
            check(got[name], c[name]["D64"], c[name]["e"], c["M64"], dd.err_dtau, f"{what}, {name}")
        else:
            check(got[name][1:], c[name]["X64"], c[name]["e"], c["M64"], dd.err_dqdd, f"{what}, {name}")
            E = fr.err_qdd(got[name][0], c[name]["qdd64"], c["M64"])
            assert E <= FACTOR * c[name]["e_qdd"], f"{what}, {name}: qdd"


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
    q = poses(kr.HandKin(ms), N, seed=21)
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
    for name in ("fd_full", "fd_free"):                                        # qdd is the forward dynamics' own result
        x = gpu_call(c["core"], c["core"].forward_dynamics, N, NJ, tau=c[name]["tau"])
        assert (bits(c["got"][name][0]) == bits(x)).all()


@pytest.mark.gpu
def test_armature_and_different_model():
    """The scaled model with general finger inertias and armatures of the size of M's diagonal: the inverse derivatives, and the
    forward ones with DEXSIM_FD_ARMATURE against -solve(M64 + diag(a), .) and without it against -solve(M64, .)."""
    sc, ms = _setup(N, model="scaled")
    hk = kr.HandKin(ms)
    arm = fr.set_armature(ms, kr.oracle_pair(sc, ms)[1], 0.5 * (hk.geom.lo + hk.geom.hi))
    q, qd = poses(hk, N, 22), ir.random_rates(N, 32)[0]
    core = _core_at(sc, ms, q, qd)
    on, off = references(sc, ms, q, qd, seed=42, arm=arm, forward=("full",)), references(sc, ms, q, qd, seed=42, forward=("full",))
    miss = dd.err_dqdd(off["fd_full"]["X64"][0], on["fd_full"]["X64"][0], on["M64"])
    print(f"armature left out: E_dqdd = {miss:.3g}, the bound is {FACTOR * on['fd_full']['e'][0]:.3g}")
    assert miss > 10 * FACTOR * on["fd_full"]["e"][0]
    del off["full"], off["noflags"], off["bias"]
    check_all(gpu_all(core, on, N, armature=True), on, "scaled model, armature")
    check_all(gpu_all(core, off, N), off, "scaled model, no armature")
    core.close()


@pytest.mark.gpu
def test_structure_free_model():
    """The model of tests/generic_model.py, which has none of the default model's exact zeros, ones and repeated numbers: the
    inverse derivatives and the forward ones with the model's own armatures, the bounds recomputed on these rows of this model."""
    sc, ms = _setup(N, model="generic", free_bodies=True)
    arm = np.array(np.ctypeslib.as_array(ms.armature), dtype=np.float64)
    q, qd = poses(kr.HandKin(ms), N, 23), ir.random_rates(N, 33)[0]
    core = _core_at(sc, ms, q, qd)
    on = references(sc, ms, q, qd, seed=43, arm=arm)
    check_all(gpu_all(core, on, N, armature=True), on, "generic model, armature")
    core.close()


def _rel(x, x64, d):
    """per pose max_r |x - x64|_r / d_r over max_r |x64|_r / d_r; the max over poses (invdyn_ref.err_tau's form)."""
    return float(((np.abs(x - x64) / d).max(1) / (np.abs(x64) / d).max(1)).max())


@pytest.mark.gpu
def test_consistency_on_the_device(posed):
    """Identities that hold on the device's own numbers, each bounded by 4 x what the float32 reference leaves of the SAME quantity.

    tau is quadratic in qd, so (tau(qd + v) - tau(qd - v)) / 2 = (d tau / d qd) v holds for a step v of qd's own size (+-3): the
    left side from dexsim_inverse_dynamics, the right side from the derivative, their difference in err_tau's form against the
    fp64 (d tau / d qd) v.
    d tau / d q at qd = 0, qdd NULL with gravity is the Hessian of the potential: |H - H^T|_rc / (d_r d_c) over the pose's largest
    |H64|_rc / (d_r d_c).  (The fp64 reference itself leaves 4e-8: the model's float32 axes and quaternions are unit to 3e-8 only,
    so what the engine and the oracle evaluate is a gradient to that order.)
    The forward route is the negated mass solve of the inverse route at the returned qdd, as numbers.  Cross-finger blocks of the
    inverse route are +0.0."""
    c = posed
    core, q, qd, M64 = c["core"], c["q"], c["qd"], c["M64"]
    d = np.sqrt(np.einsum("nii->ni", M64))
    hk, links, grav = c["hk"], c["links"], c["grav"]
    v = ir.random_rates(N, seed=61)[0]
    tau = lambda vel: gpu_call(core, core.inverse_dynamics, N, NJ, qdd=c["qdd"], q=q, qd=vel)
    lhs = 0.5 * (tau(qd + v).astype(np.float64) - tau(qd - v).astype(np.float64))
    rhs = np.einsum("nrc,nc->nr", jac(c["got"]["full"][1]).astype(np.float64), v.astype(np.float64))
    want = np.einsum("nrc,nc->nr", c["full"]["D64"][1], v.astype(np.float64))
    r32 = lambda vel: dd.id_derivatives(hk, links, q, vel, c["qdd"], grav, f32)[0]
    lhs32 = f32(0.5) * (r32(qd + v) - r32(qd - v))
    rhs32 = np.einsum("nrc,nc->nr", c["full"]["D32"][1], v)
    assert lhs32.dtype == f32 and rhs32.dtype == f32
    E, e = _rel(lhs - rhs + want, want, d), _rel(lhs32.astype(np.float64) - rhs32 + want, want, d)
    print(f"(tau(qd + v) - tau(qd - v)) / 2 against (d tau / d qd) v: {E:.3g} (fp32 reference {e:.3g}, bound {FACTOR * e:.3g})")
    assert E <= FACTOR * e
    z = np.zeros_like(qd)
    H = jac(gpu_idd(core, N, q=q, qd=z, which=(True, False))[0]).astype(np.float64)
    H64, H32 = (dd.id_derivatives(hk, links, q, z, None, grav, dt)[1].astype(np.float64) for dt in (np.float64, f32))
    dd2 = d[:, :, None] * d[:, None, :]
    asym = lambda A: float(((np.abs(A - A.transpose(0, 2, 1)) / dd2).max(axis=(1, 2)) / (np.abs(H64) / dd2).max(axis=(1, 2))).max())
    print(f"asymmetry of the potential's Hessian: {asym(H):.3g} (fp32 reference {asym(H32):.3g}, fp64 {asym(H64):.3g})")
    assert asym(H64) <= 1e-7 and asym(H) <= FACTOR * asym(H32)
    for name in ("fd_full", "fd_free"):
        qdd, Xq, Xv = c["got"][name]
        Dq, Dv = gpu_idd(core, N, qdd=qdd)
        for X, D in ((Xq, Dq), (Xv, Dv)):
            S = gpu_call(core, core.mass_solve, N, NJ, NJ, rhs=D)
            assert np.array_equal(X, -S), name                                 # as numbers: -0 == +0
    for D in c["got"]["full"]:
        for f in range(5):
            for g in range(5):
                if f != g:
                    assert (bits(D[:, 6 + 4 * f:10 + 4 * f, 6 + 4 * g:10 + 4 * g]) == 0).all()   # +0.0, not -0.0, not untouched


@pytest.mark.gpu
def test_addressing(posed):
    import torch
    c = posed
    core, q, qd, qdd, got = c["core"], c["q"], c["qd"], c["qdd"], c["got"]
    tau = c["fd_full"]["tau"]
    eq = lambda a, b: all((bits(x) == bits(y)).all() for x, y in zip(a, b))
    ids = [69, 0, 64, 3, 63]                                                   # out of order; qdd / tau ride with the output rows
    assert eq(gpu_idd(core, 5, qdd=qdd[ids], env_ids=ids), [g[ids] for g in got["full"]])
    assert eq(gpu_idd(core, 5, env_ids=ids), [g[ids] for g in got["bias"]])
    assert eq(gpu_fdd(core, 5, tau=tau[ids], env_ids=ids), [g[ids] for g in got["fd_full"]])
    assert eq(gpu_idd(core, 1, qdd=qdd[[37]], env_ids=[37]), [g[[37]] for g in got["full"]])          # k = 1
    assert eq(gpu_fdd(core, 1, tau=tau[[37]], env_ids=[37]), [g[[37]] for g in got["fd_full"]])
    # overrides at k = 64, 65 (the workgroup boundary): rows copied from env state are the state path's bits
    for k in (64, 65):
        assert eq(gpu_idd(core, k, qdd=qdd[:k], q=q[:k], qd=qd[:k], env_ids=[-1]), [g[:k] for g in got["full"]])
        assert eq(gpu_fdd(core, k, tau=tau[:k], q=q[:k], qd=qd[:k]), [g[:k] for g in got["fd_full"]])
    # k = 130 (three workgroups): the state rows again, the rest meet the reference
    n_new = 130 - N
    qn = poses(c["hk"], n_new, seed=23)
    vn = ir.random_rates(n_new, seed=24)[0]
    cn = references(c["sc"], core.model, qn, vn, seed=25, forward=("full",))
    src = np.concatenate([np.arange(40), np.full(n_new, -1), np.arange(40, N)])
    st = src >= 0
    cat = lambda old, new: np.concatenate([old[:40], new, old[40:]])
    oi = gpu_idd(core, 130, qdd=cat(qdd, cn["qdd"]), q=cat(q, qn), qd=cat(qd, vn))
    of = gpu_fdd(core, 130, tau=cat(tau, cn["fd_full"]["tau"]), q=cat(q, qn), qd=cat(qd, vn))
    assert eq([o[st] for o in oi], [g[src[st]] for g in got["full"]]) and eq([o[st] for o in of], [g[src[st]] for g in got["fd_full"]])
    check_all(dict(full=[o[~st] for o in oi], fd_full=[o[~st] for o in of]), cn, "overrides")
    # rows permuted give permuted bits
    perm = np.random.default_rng(7).permutation(N)
    assert eq(gpu_idd(core, N, qdd=qdd[perm], q=q[perm], qd=qd[perm]), [g[perm] for g in got["full"]])
    assert eq(gpu_fdd(core, N, tau=tau[perm], q=q[perm], qd=qd[perm]), [g[perm] for g in got["fd_full"]])
    # ids outside [0, N) leave their rows as they are
    bad = [5, -1, N, 69]
    for o, g in zip(gpu_idd(core, 4, qdd=qdd[[5, 0, 0, 69]], env_ids=bad), got["full"]):
        assert np.isnan(o[1:3]).all() and (bits(o[[0, 3]]) == bits(g[[5, 69]])).all()
    for o, g in zip(gpu_fdd(core, 4, tau=tau[[5, 0, 0, 69]], env_ids=bad), got["fd_full"]):
        assert np.isnan(o[1:3]).all() and (bits(o[[0, 3]]) == bits(g[[5, 69]])).all()
    # each output alone has the bits it has next to the other
    for which in ((True, False), (False, True)):
        a, b = gpu_idd(core, N, qdd=qdd, which=which), gpu_fdd(core, N, tau=tau, which=which)
        for i in (0, 1):
            if which[i]:
                assert (bits(a[i]) == bits(got["full"][i])).all() and (bits(b[1 + i]) == bits(got["fd_full"][1 + i])).all()
        assert (bits(b[0]) == bits(got["fd_full"][0])).all()
    # argument errors come back as DEXSIM_ERR_ARG with their message, before any launch
    lib, h = core.lib, core.h
    out = torch.full((3, 130, NJ, NJ), float("nan"), device=core.device)
    p0, p1, p2, pm = [C.c_void_p(out[i].data_ptr()) for i in (0, 1, 2)] + [C.c_void_p(out.data_ptr() + 2)]
    keep = [_dev(a) for a in (cat(q, qn), cat(qd, vn))]
    pq, pv = (C.c_void_p(t.data_ptr()) for t in keep)
    idd, fdd = lib.dexsim_inverse_dynamics_derivatives, lib.dexsim_forward_dynamics_derivatives

    def refused(rc, text):
        assert rc == 1 and text in lib.dexsim_last_error(), (rc, lib.dexsim_last_error())
    refused(idd(h, None, 0, None, None, None, 1, p0, p1, None), b"k must be positive")
    refused(idd(h, None, N - 1, None, None, None, 1, p0, p1, None), b"k == num_envs")
    refused(idd(h, None, 130, pq, None, None, 1, p0, p1, None), b"q and qd")
    refused(idd(h, None, N, None, pv, None, 1, p0, p1, None), b"q and qd")
    refused(idd(h, None, N, None, None, None, 2, p0, p1, None), b"flag")
    refused(idd(h, None, N, None, None, None, 1, None, None, None), b"at least one")
    refused(idd(h, None, N, None, None, None, 1, pm, p1, None), b"dtau_dq")
    refused(idd(h, None, N, None, None, None, 1, None, pm, None), b"dtau_dqd")
    refused(fdd(h, None, 0, None, None, None, 1, p0, p1, p2, None), b"k must be positive")
    refused(fdd(h, None, N - 1, None, None, None, 1, p0, p1, p2, None), b"k == num_envs")
    refused(fdd(h, None, 130, pq, None, None, 1, p0, p1, p2, None), b"q and qd")
    refused(fdd(h, None, N, None, pv, None, 1, p0, p1, p2, None), b"q and qd")
    refused(fdd(h, None, N, None, None, None, 4, p0, p1, p2, None), b"flag")
    refused(fdd(h, None, N, None, None, None, 3, None, p1, p2, None), b"qdd")
    refused(fdd(h, None, N, None, None, None, 3, pm, p1, p2, None), b"qdd")
    refused(fdd(h, None, N, None, None, None, 3, p0, None, None, None), b"at least one")
    refused(fdd(h, None, N, None, None, None, 3, p0, pm, None, None), b"dqdd_dq")
    refused(fdd(h, None, N, None, None, None, 3, p0, p1, pm, None), b"dqdd_dqd")
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                                              # nothing was launched


@pytest.mark.gpu
def test_purity():
    import torch
    rng = np.random.default_rng(41)
    qdd, tau = rng.uniform(-1, 1, (N, NJ)).astype(f32), rng.uniform(-1, 1, (N, NJ)).astype(f32)
    rnd = lambda *s: torch.rand(*s, device="cuda:0")

    def between(core):
        gpu_idd(core, 3, env_ids=[69, 1, 64], gravity=False, which=(False, True))
        gpu_fdd(core, 3, env_ids=[69, 1, 64], gravity=False, armature=True, which=(True, False))
        gpu_idd(core, 100, q=rnd(100, NJ), qd=rnd(100, NJ), qdd=rnd(100, NJ))
        gpu_fdd(core, 100, q=rnd(100, NJ), qd=rnd(100, NJ), tau=rnd(100, NJ))
    got = purity_frame(lambda core: [*gpu_idd(core, N, qdd=qdd), *gpu_fdd(core, N, tau=tau)], between, n=N)
    a1, b1 = got[:2], got[2:]                                                  # (dtau_dq, dtau_dqd), (qdd, dqdd_dq, dqdd_dqd)
    assert len(b1) == 3 and not any(np.isnan(x).any() for x in a1 + b1) and np.abs(a1[0]).max() > 0 and np.abs(b1[1]).max() > 0


@pytest.mark.gpu
def test_public_surface():
    """The views the env returns are Jacobians: D[i] @ dq is the first-order change of get_inverse_dynamics from q to q + dq, and
    the forward call's derivative is the chain rule of the public calls.  dq is uniform in +-1e-2 on every coordinate: large
    enough that what is left of the change after the first-order term is the second-order remainder (about 1e-2 of the change) and
    not the roundoff of the two float32 forces that are subtracted (about 1e-4 of it).  The bound is 4 x what the fp64 reference
    leaves for the same dq, its second-order remainder, in err_tau's form against the fp64 first-order change; the transposed
    array misses it."""
    import torch
    from dexrobot_isaac_amd import make_env
    env = make_env("BlindGrasping", N, "cuda:0", "cuda:0", 0)
    env.reset()
    g = torch.Generator().manual_seed(6)
    for _ in range(3):                                                         # some joint velocity
        env.step((2 * torch.rand(N, env.num_actions, generator=g) - 1).cuda())
    core = env._core
    q0, v0 = env.dof_pos.clone(), env.dof_vel.clone()
    qdd = (20 * torch.rand(N, NJ, generator=g) - 10).cuda()
    dq = (2e-2 * torch.rand(N, NJ, generator=g) - 1e-2).cuda()
    Dq, Dv = env.get_inverse_dynamics_derivatives(qdd)
    assert Dq.shape == (N, NJ, NJ) and Dv.shape == (N, NJ, NJ) and not Dq.is_contiguous()
    assert not torch.isnan(Dq).any() and not torch.isnan(Dv).any()
    fa, oa = _guarded(N, NJ, NJ)
    fb, ob = _guarded(N, NJ, NJ)
    Eq, Ev = env.get_inverse_dynamics_derivatives(qdd, out=(oa, ob))
    _guards_ok(fa)
    _guards_ok(fb)
    assert Eq.data_ptr() == oa.data_ptr() and torch.equal(Eq.view(torch.int32), Dq.view(torch.int32)) and torch.equal(oa.transpose(1, 2), Eq)
    sub = env.get_inverse_dynamics_derivatives(qdd[[3, 1]], env_ids=[3, 1])
    assert torch.equal(sub[0].view(torch.int32), Dq[[3, 1]].view(torch.int32)) and torch.equal(sub[1].view(torch.int32), Dv[[3, 1]].view(torch.int32))
    over = env.get_inverse_dynamics_derivatives(qdd, q=q0, qd=v0)                # the overrides at the current state: the state path's bits
    assert torch.equal(over[0].view(torch.int32), Dq.view(torch.int32))
    with pytest.raises(ValueError):
        env.get_inverse_dynamics_derivatives(q=q0)
    # first order, against the existing call
    M64 = env.get_mass_matrix().double().cpu().numpy()
    d = np.sqrt(np.einsum("nii->ni", M64))
    hk, links = kr.HandKin(core.model), dd.Links(core.model)
    grav = np.array(core.cfg.gravity, dtype=np.float64)
    qn, vn, an, dn = (t.cpu().numpy() for t in (q0, v0, qdd, dq))
    t64, D64, _ = dd.id_derivatives(hk, links, qn, vn, an, grav)
    t64b = dd.id_derivatives(hk, links, qn.astype(np.float64) + dn, vn, an, grav)[0]
    first64 = np.einsum("nrc,nc->nr", D64, dn.astype(np.float64))
    rem64 = _rel(t64b - t64, first64, d)
    bound = FACTOR * rem64
    change = (env.get_inverse_dynamics(qdd, q=q0 + dq, qd=v0) - env.get_inverse_dynamics(qdd)).double().cpu().numpy()
    first = torch.einsum("nrc,nc->nr", Dq.double(), dq.double()).cpu().numpy()
    E = _rel(change - first + first64, first64, d)
    print(f"D @ dq against the change of get_inverse_dynamics: {E:.3g}; fp64 second-order remainder {rem64:.3g}, bound {bound:.3g}")
    assert E <= bound
    Et = _rel(change - torch.einsum("ncr,nc->nr", Dq.double(), dq.double()).cpu().numpy() + first64, first64, d)
    assert Et > bound                                                          # the transposed array does not pass
    # the forward call: shapes, views, outputs given, and the acceleration of get_forward_dynamics
    tau = env.get_inverse_dynamics(qdd)
    acc, Xq, Xv = env.get_forward_dynamics_derivatives(tau)
    assert acc.shape == (N, NJ) and Xq.shape == (N, NJ, NJ) and Xv.shape == (N, NJ, NJ)
    assert torch.equal(acc.view(torch.int32), env.get_forward_dynamics(tau).view(torch.int32))
    assert not torch.isnan(Xq).any() and not torch.isnan(Xv).any()
    fc, oc = _guarded(N, NJ)
    trip = env.get_forward_dynamics_derivatives(tau, out=(oc, oa, ob))
    for f in (fa, fb, fc):
        _guards_ok(f)
    assert trip[0] is oc and trip[1].data_ptr() == oa.data_ptr() and torch.equal(trip[1].view(torch.int32), Xq.view(torch.int32))
    # d qdd / d q by the chain rule: -M^-1 (d tau / d q) at the returned acceleration, through the public calls
    Dq2, _ = env.get_inverse_dynamics_derivatives(acc)
    S = env.solve_mass_matrix(Dq2.transpose(1, 2).contiguous())
    assert torch.equal(Xq.transpose(1, 2), -S)
    env.close()
