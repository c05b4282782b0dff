"""Float64 references for the derivatives of the inverse and the forward dynamics (dexsim_inverse_dynamics_derivatives,
dexsim_forward_dynamics_derivatives) and the error metrics of tests/test_dynamics_derivatives.py.

`id_derivatives` is an analytic derivative of the Newton-Euler recursion in numpy over kindyn_ref.HandKin (the tree, axes and offsets
of its HandGeometry; link masses, centres and inertias of the model struct; joint frames by `frames` below, the header's formula
evaluated as the engine and the oracle evaluate it): next to the motion (w, al, ao) of every joint frame it carries, for all 52
directions at once (26 of q, 26 of qd), the derivative of that motion and the frame's virtual rotation th (d U = [th] x U), forms
every link's wrench and its derivative about the frame origin, and sums them up the tree.  It shares no code with the engine and
takes `dtype` like invdyn_ref.bias_accel, so the SAME code evaluated in float32 gives the roundoff figure the tolerances are 4 x of.
tests/test_dynamics_derivatives.py checks its float64 evaluation against central differences of the fp64 CPU oracle
(tau = M qdd + b of Oracle.mass_matrix).

Matrices here are Jacobians: D[n, r, c] = d (tau or qdd)_r / d (q or qd)_c.  The device writes the transpose (derivative-major).

The forward-dynamics derivative is -solve(M [+ diag a], d tau / d .) at the acceleration the forward dynamics returns:
fwddyn_ref.solve64 in float64, fwddyn_ref.chol_solve in float32 for the roundoff figure.
"""
import numpy as np

from tests import fwddyn_ref as fr
from tests import kindyn_ref as kr

NJ = kr.NJ


class Links:
    """Masses, centres (joint frame) and inertias about the centre (joint-frame axes, 3 x 3) of the 26 links, as float64."""

    def __init__(self, ms):
        A = lambda x: np.array(np.ctypeslib.as_array(x), dtype=np.float64)
        self.mass, self.com = A(ms.mass), A(ms.com)
        s = A(ms.inertia)                                                      # xx yy zz xy xz yz
        self.inertia = np.stack([np.array([[v[0], v[3], v[4]], [v[3], v[1], v[5]], [v[4], v[5], v[2]]]) for v in s])


def _qmul(a, b):
    """xyzw Hamilton product of (n, 4) quaternions."""
    ax, ay, az, aw = a.T
    bx, by, bz, bw = b.T
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], axis=1)


def _q2mat(q):
    """The header's matrix of (n, 4) quaternions, NOT normalised first: for |q|^2 = 1 - k it is (1 - k) U + k I with U the rotation."""
    x, y, z, w = q.T
    one = np.ones_like(x)
    return np.stack([np.stack([one - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=1),
                     np.stack([2 * (x * y + z * w), one - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), one - 2 * (x * x + y * y)], axis=1)], axis=1)


def frames(hk, q, dtype=np.float64):
    """The joint frames of the poses q (n, 26) by the header's joint-frame formula as the engine and the oracle evaluate it:
    quaternions are multiplied along the chain and turned into matrices WITHOUT normalising, so with the float32 jqoff of the
    model (|q| = 1 +- 6e-8) a frame's matrix is R = (1 - k) U + k I, U a rotation, k = 1 - |q|^2.  HandGeometry.fk normalises
    and differs from the oracle by 1e-7 in the derivatives, more than the 1e-7 the validation allows.
    Returns o (n, 26, 3) origins, R (n, 26, 3, 3), a (n, 26, 3) world axes, lever (n, 26, 3) = R_parent poff, k (n, 26)."""
    g = hk.geom
    q = np.asarray(q, dtype=dtype)
    n = len(q)
    quat, o, R, a, lever, k = ([None] * NJ for _ in range(6))
    for j in range(NJ):
        p = g.parent(j)
        qp = np.broadcast_to(g.spawn_quat.astype(dtype), (n, 4)) if p < 0 else quat[p]
        op = np.broadcast_to(g.spawn_pos.astype(dtype), (n, 3)) if p < 0 else o[p]
        Rp = _q2mat(qp) if p < 0 else R[p]
        ax = g.jaxis[j].astype(dtype)
        lever[j] = np.einsum("nik,k->ni", Rp, g.jpoff[j].astype(dtype))
        qz = _qmul(qp, np.broadcast_to(g.jqoff[j].astype(dtype), (n, 4)))
        a[j] = np.einsum("nik,k->ni", _q2mat(qz), ax)
        if g.jtype[j] == 0:
            quat[j], o[j] = qz, op + lever[j] + q[:, j, None] * a[j]
        else:
            h = dtype(0.5) * q[:, j]
            quat[j], o[j] = _qmul(qz, np.concatenate([ax[None] * np.sin(h)[:, None], np.cos(h)[:, None]], axis=1)), op + lever[j]
        R[j] = _q2mat(quat[j])
        k[j] = 1 - (quat[j] * quat[j]).sum(1)
    st = lambda x: np.stack(x, axis=1)
    out = tuple(st(x) for x in (o, R, a, lever, k))
    assert all(x.dtype == dtype for x in out)
    return out


def _x(a, b):
    return np.cross(a, b)


def id_derivatives(hk, links, q, qd, qdd, gravity, dtype=np.float64, fr_=None):
    """(tau (n, 26), d tau / d q (n, 26, 26), d tau / d qd (n, 26, 26)) of tau = M(q) qdd + c(q, qd) + g(q) for the gravity
    vector `gravity` (None = no gravity) and qdd (None = zero), every operation in `dtype`.  fr_: frames(hk, q, dtype), if the
    caller has them.

    A frame's virtual rotation th turns U, not R: d (R v) = th x (R v - k v) for a vector v fixed in the frame, and a hinge turns
    its frame about the unit axis (a - k axis) / (1 - k), while the velocity it adds is along a = R axis itself."""
    g = hk.geom
    o, R, A, LV, K = frames(hk, q, dtype) if fr_ is None else fr_
    n, nd = len(q), 2 * NJ
    q = np.asarray(q, dtype=dtype)
    qd = np.asarray(qd, dtype=dtype)
    qdd = np.zeros((n, NJ), dtype=dtype) if qdd is None else np.asarray(qdd, dtype=dtype)
    a0 = np.zeros((n, 3), dtype=dtype) if gravity is None else np.broadcast_to(-np.asarray(gravity, dtype=dtype), (n, 3))
    E = lambda v: v[:, None, :]                                                # a primal vector next to the 52 tangents
    S = lambda s: s[:, None, None]                                             # a per-pose scalar next to the tangents
    P0, T0 = np.zeros((n, 3), dtype=dtype), np.zeros((n, nd, 3), dtype=dtype)
    w, al, ao, a, r = ([None] * NJ for _ in range(5))
    th, dw, dal, dao, da, dr = ([None] * NJ for _ in range(6))
    for j in range(NJ):
        p = g.parent(j)
        sq, sv = np.zeros((1, nd, 1), dtype=dtype), np.zeros((1, nd, 1), dtype=dtype)   # the direction's component on joint j
        sq[0, j], sv[0, NJ + j] = 1, 1
        ax, poff = g.jaxis[j].astype(dtype), g.jpoff[j].astype(dtype)
        aj, kj = A[:, j], K[:, j, None]
        if p < 0:                                                              # the spawn frame neither moves nor turns
            wp, alp, aop, thp, dwp, dalp, daop, rj, kp = P0, P0, a0, T0, T0, T0, T0, P0, 0 * kj
        else:
            wp, alp, aop, thp, dwp, dalp, daop, rj, kp = w[p], al[p], ao[p], th[p], dw[p], dal[p], dao[p], o[:, j] - o[:, p], K[:, p, None]
        slide = g.jtype[j] == 0
        daj = _x(thp, E(aj - kj * ax))
        drj = _x(thp, E(LV[:, j] - kp * poff))
        if slide:
            drj = drj + sq * E(aj) + S(q[:, j]) * daj
        wxr = _x(wp, rj)
        base = aop + _x(alp, rj) + _x(wp, wxr)                                 # the parent's point under o_j
        dbase = daop + _x(dalp, E(rj)) + _x(E(alp), drj) + _x(dwp, E(wxr)) + _x(E(wp), _x(dwp, E(rj)) + _x(E(wp), drj))
        wxa = _x(wp, aj)
        dwxa = _x(dwp, E(aj)) + _x(E(wp), daj)
        vj, cj = qd[:, j, None], qdd[:, j, None]
        if slide:
            w[j], al[j], ao[j] = wp, alp, base + dtype(2) * vj * wxa + cj * aj
            dw[j], dal[j], th[j] = dwp, dalp, thp
            dao[j] = dbase + dtype(2) * sv * E(wxa) + dtype(2) * S(qd[:, j]) * dwxa + S(qdd[:, j]) * daj
        else:
            w[j], al[j], ao[j] = wp + vj * aj, alp + vj * wxa + cj * aj, base
            dw[j] = dwp + sv * E(aj) + S(qd[:, j]) * daj
            dal[j] = dalp + sv * E(wxa) + S(qd[:, j]) * dwxa + S(qdd[:, j]) * daj
            dao[j], th[j] = dbase, thp + sq * E((aj - kj * ax) / (1 - kj))
        a[j], r[j], da[j], dr[j] = aj, rj, daj, drj
    F, Nm, dF, dN = ([None] * NJ for _ in range(4))
    I3 = np.eye(3, dtype=dtype)
    for j in range(NJ):                                                        # every link's wrench about its frame's origin
        Rj, thj = R[:, j], th[j]
        Rk = Rj - K[:, j, None, None] * I3                                     # d R = [th] x Rk
        m = dtype(links.mass[j])
        Ib, com = links.inertia[j].astype(dtype), links.com[j].astype(dtype)
        rc = np.einsum("nik,k->ni", Rj, com)
        I = np.einsum("nik,kl,njl->nij", Rj, Ib, Rj)
        Ik = np.einsum("nik,kl,njl->nij", Rk, Ib, Rj)                          # Rk Ib R^T; its transpose is R Ib Rk^T
        Ip = lambda v: np.einsum("nij,nj->ni", I, v)
        It = lambda v: np.einsum("nij,ndj->ndi", I, v)
        dI = lambda v: _x(thj, E(np.einsum("nij,nj->ni", Ik, v))) - np.einsum("nji,ndj->ndi", Ik, _x(thj, E(v)))   # (d I) v
        drc = _x(thj, E(np.einsum("nik,k->ni", Rk, com)))
        wxrc = _x(w[j], rc)
        ac = ao[j] + _x(al[j], rc) + _x(w[j], wxrc)
        dac = dao[j] + _x(dal[j], E(rc)) + _x(E(al[j]), drc) + _x(dw[j], E(wxrc)) + _x(E(w[j]), _x(dw[j], E(rc)) + _x(E(w[j]), drc))
        f, df = m * ac, m * dac
        Iw = Ip(w[j])
        F[j], dF[j] = f, df
        Nm[j] = Ip(al[j]) + _x(w[j], Iw) + _x(rc, f)
        dN[j] = dI(al[j]) + It(dal[j]) + _x(dw[j], E(Iw)) + _x(E(w[j]), dI(w[j]) + It(dw[j])) + _x(drc, E(f)) + _x(E(rc), df)
    tau = np.zeros((n, NJ), dtype=dtype)
    D = np.zeros((n, NJ, nd), dtype=dtype)
    for j in range(NJ - 1, -1, -1):                                            # children before parents: parent(j) < j
        X, dX = (F[j], dF[j]) if g.jtype[j] == 0 else (Nm[j], dN[j])
        tau[:, j] = (a[j] * X).sum(-1)
        D[:, j] = (da[j] * E(X)).sum(-1) + (dX * E(a[j])).sum(-1)
        p = g.parent(j)
        if p >= 0:
            dN[p] = dN[p] + dN[j] + _x(dr[j], E(F[j])) + _x(E(r[j]), dF[j])
            Nm[p] = Nm[p] + Nm[j] + _x(r[j], F[j])
            F[p], dF[p] = F[p] + F[j], dF[p] + dF[j]
    assert tau.dtype == dtype and D.dtype == dtype
    return tau, D[:, :, :NJ], D[:, :, NJ:]


def oracle_tau(orc, q, qd, qdd):
    """tau = M(q) qdd + b(q, qd) of the oracle for one pose, in float64 (qdd None = zero)."""
    M, b = orc.mass_matrix(np.asarray(q, dtype=np.float64), np.asarray(qd, dtype=np.float64))
    return b if qdd is None else M @ np.asarray(qdd, dtype=np.float64) + b


def central_differences(orc, q, qd, qdd, h_q, h_qd):
    """(d tau / d q, d tau / d qd) (n, 26, 26) by central differences of oracle_tau with the steps h_q and h_qd."""
    n = len(q)
    Dq, Dv = np.zeros((n, NJ, NJ)), np.zeros((n, NJ, NJ))
    for i in range(n):
        qi, vi = np.asarray(q[i], dtype=np.float64), np.asarray(qd[i], dtype=np.float64)
        ai = None if qdd is None else qdd[i]
        for c in range(NJ):
            e = np.zeros(NJ)
            e[c] = 1.0
            Dq[i, :, c] = (oracle_tau(orc, qi + h_q * e, vi, ai) - oracle_tau(orc, qi - h_q * e, vi, ai)) / (2 * h_q)
            Dv[i, :, c] = (oracle_tau(orc, qi, vi + h_qd * e, ai) - oracle_tau(orc, qi, vi - h_qd * e, ai)) / (2 * h_qd)
    return Dq, Dv


def fd_derivatives(A, Dq, Dv, dtype=np.float64):
    """-(A)^-1 D for A = M [+ diag a] (n, 26, 26) and the Jacobians Dq, Dv of the inverse dynamics: numpy.linalg.solve in
    float64, fwddyn_ref.chol_solve in float32."""
    if dtype == np.float64:
        return -fr.solve64(A, Dq), -fr.solve64(A, Dv)
    return -fr.chol_solve(A, Dq, dtype), -fr.chol_solve(A, Dv, dtype)


def _err(D, D64, scale):
    D, D64 = np.asarray(D, dtype=np.float64), np.asarray(D64, dtype=np.float64)
    num = (np.abs(D - D64) * scale).max(axis=(1, 2))
    den = (np.abs(D64) * scale).max(axis=(1, 2))
    return float((num / den).max())


def err_dtau(D, D64, M64):
    """E_dtau: per pose max_rc |D - D64|_rc / d_r over max_rc |D64|_rc / d_r with d_r = sqrt(M64_rr); the max over poses.  A pose
    counts as a whole: the slide columns of d tau / d q are analytically zero."""
    return _err(D, D64, 1.0 / np.sqrt(np.einsum("nii->ni", M64))[:, :, None])


def err_dqdd(D, D64, M64):
    """E_dqdd: err_dtau with the dual scaling, |.|_rc d_r (fwddyn_ref.err_qdd's)."""
    return _err(D, D64, np.sqrt(np.einsum("nii->ni", M64))[:, :, None])
