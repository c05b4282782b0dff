"""Float64 references for the inverse dynamics and the bias accelerations (dexsim_inverse_dynamics, dexsim_body_bias_accel) and the
error metrics of tests/test_inverse_dynamics.py.

tau comes from the CPU oracle (oracle/dexsim_oracle.c: crba and rnea_bias behind Oracle.mass_matrix(q, qd)): tau = M qdd + b, where
the oracle's bias b includes gravity; the velocity-product force alone comes from an oracle pair built from a config whose gravity
is zero, directly and not as a difference of two results.  The fp32 and fp64 builds of the oracle give the roundoff figure e_tau.
The bias accelerations Jdot qd are a numpy recursion over kindyn_ref.HandKin.body_frames that takes `dtype` like HandKin.jacobian,
so the SAME code evaluated in float32 gives e_acc; test_inverse_dynamics checks it against central differences of the Jacobian.
"""
import numpy as np

from dexrobot_isaac_amd.config import build_sim_config, default_cfg
from tests import kindyn_ref as kr

NB, NJ = kr.NB, kr.NJ


def zero_gravity_config(n, task="BlindGrasping"):
    """The sim config of query_rig.setup(n, task) with gravity (0, 0, 0)."""
    cfg = default_cfg(task)
    cfg["env"]["numEnvs"] = n
    cfg["sim"]["gravity"] = [0.0, 0.0, 0.0]
    return build_sim_config(cfg)[0]


def random_rates(n, seed, qd_range=3.0, qdd_range=10.0):
    """qd uniform in +-3 (m/s for the slides, rad/s otherwise) and qdd uniform in +-10, rounded to float32."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-qd_range, qd_range, (n, NJ)).astype(np.float32), rng.uniform(-qdd_range, qdd_range, (n, NJ)).astype(np.float32))


def mass_bias(orc, q, qd):
    """M (n, 26, 26) and the bias force b (n, 26) of the oracle at (q, qd), as float64 arrays (values of the oracle's own precision)."""
    M = np.zeros((len(q), NJ, NJ))
    b = np.zeros((len(q), NJ))
    for i in range(len(q)):
        M[i], b[i] = orc.mass_matrix(np.asarray(q[i], dtype=np.float64), np.asarray(qd[i], dtype=np.float64))
    return M, b


def tau_of(M, b, qdd, dtype=np.float64):
    """M @ qdd + b formed in `dtype` (qdd None = zero)."""
    M, b = np.asarray(M, dtype=dtype), np.asarray(b, dtype=dtype)
    if qdd is None:
        return b
    return np.einsum("nij,nj->ni", M, np.asarray(qdd, dtype=dtype)) + b


def err_tau(tau, tau64, M64):
    """kindyn_ref.err_g's form: per pose max_j |tau - tau64|_j / sqrt(M64_jj) over max_j |tau64|_j / sqrt(M64_jj); the max over poses."""
    return kr.err_g(tau, tau64, M64)


def bias_accel(hk, q, qd, dtype=np.float64):
    """(37, 6) Jdot qd of the hand bodies at (q, qd): world linear acceleration of the body origin and angular acceleration at
    qdd = 0, without gravity.  Newton-Euler kinematics in world axes: (w, al, ao) of every joint frame, ao the classical
    acceleration of its origin."""
    g = hk.geom
    p, _, o, R = hk.body_frames(q, dtype)
    qd = np.asarray(qd, dtype=dtype)
    w, al, ao = (np.zeros((NJ, 3), dtype=dtype) for _ in range(3))
    zero = np.zeros(3, dtype=dtype)
    for j in range(NJ):
        pj = g.parent(j)
        wp, alp, aop, r = (zero, zero, zero, zero) if pj < 0 else (w[pj], al[pj], ao[pj], o[j] - o[pj])
        a = R[j] @ g.jaxis[j].astype(dtype)
        ao[j] = aop + np.cross(alp, r) + np.cross(wp, np.cross(wp, r))       # the parent's point under o_j
        if g.jtype[j] == 0:
            w[j], al[j] = wp, alp
            ao[j] = ao[j] + dtype(2) * qd[j] * np.cross(wp, a)
        else:
            w[j] = wp + qd[j] * a
            al[j] = alp + qd[j] * np.cross(wp, a)
    acc = np.zeros((NB, 6), dtype=dtype)
    for b in range(NB):
        j = int(hk.body_parent[b])
        if j < 0:
            continue
        r = p[b] - o[j]
        acc[b, 0:3] = ao[j] + np.cross(al[j], r) + np.cross(w[j], np.cross(w[j], r))
        acc[b, 3:6] = al[j]
    return acc


def err_acc(acc, acc64):
    """(linear, angular): per pose the maximum absolute error over bodies over the maximum absolute reference value of the pose
    (a pose whose reference is 0 is compared absolutely against 0); the max over poses."""
    acc, acc64 = np.asarray(acc, dtype=np.float64), np.asarray(acc64, dtype=np.float64)
    out = []
    for sl in (slice(0, 3), slice(3, 6)):
        num = np.abs(acc[:, :, sl] - acc64[:, :, sl]).max(axis=(1, 2))
        den = np.abs(acc64[:, :, sl]).max(axis=(1, 2))
        out.append(float(np.where(den > 0, num / np.where(den > 0, den, 1.0), num).max()))
    return tuple(out)


FACTOR = 4                 # the device may miss the fp64 reference by this many times the fp32 reference's own error


def gpu_tau(core, k, qdd=None, env_ids=None, q=None, qd=None, gravity=True):
    """core.inverse_dynamics into a guarded output (tests/query_rig.py), as a numpy array."""
    from tests.query_rig import dev, guarded, guards_ok
    full, out = guarded(k, NJ)
    core.inverse_dynamics(out, qdd=dev(qdd), env_ids=env_ids, q=dev(q), qd=dev(qd), gravity=gravity)
    guards_ok(full)
    return out.cpu().numpy()


def check_tau(tau, tau64, M64, e, what):
    assert not np.isnan(tau).any(), f"{what}: an element was not written"
    E = err_tau(tau, tau64, M64)
    print(f"{what}: E_tau = {E:.3g} (fp32 oracle: {e:.3g}, bound {FACTOR * e:.3g})")
    assert E <= FACTOR * e
