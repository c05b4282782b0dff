"""Float64 references for the forward dynamics and the mass-matrix solves (dexsim_forward_dynamics, dexsim_mass_solve) and the
error metrics of tests/test_forward_dynamics.py.

M64 and the bias force b64 = c + g come from the fp64 CPU oracle through invdyn_ref.mass_bias; qdd64 = solve(M64 [+ diag(a)],
tau - b64) by numpy.linalg.solve.  The fp32 reference the tolerances are 4 x of is `chol_solve` below, a Cholesky written out in
numpy and run in float32 on the fp32 oracle's M32 and b32; the same code in float64 is checked against numpy.linalg.solve.
"""
import numpy as np

from tests import invdyn_ref as ir
from tests import kindyn_ref as kr

NJ = kr.NJ


def chol_solve(M, b, dtype=np.float64):
    """x with M x = b for SPD M (n, 26, 26) and b (n, 26) or (n, 26, r): Cholesky and two triangular solves, every operation in
    `dtype` (the dot products accumulate in dtype too: the operands are dtype arrays)."""
    M, b = np.asarray(M, dtype=dtype), np.asarray(b, dtype=dtype)
    vec = b.ndim == 2
    if vec:
        b = b[:, :, None]
    n, m = M.shape[0], M.shape[1]
    L = np.zeros_like(M)
    for j in range(m):
        s = M[:, j, j] - (L[:, j, :j] * L[:, j, :j]).sum(1, dtype=dtype)
        L[:, j, j] = np.sqrt(s)
        for i in range(j + 1, m):
            L[:, i, j] = (M[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(1, dtype=dtype)) / L[:, j, j]
    y = np.zeros_like(b)
    for i in range(m):
        y[:, i] = (b[:, i] - np.einsum("nk,nkr->nr", L[:, i, :i], y[:, :i]).astype(dtype)) / L[:, i, i, None]
    x = np.zeros_like(b)
    for i in range(m - 1, -1, -1):
        x[:, i] = (y[:, i] - np.einsum("nk,nkr->nr", L[:, i + 1:, i], x[:, i + 1:]).astype(dtype)) / L[:, i, i, None]
    assert x.dtype == dtype
    return x[:, :, 0] if vec else x


def solve64(M64, rhs, arm=None):
    """numpy.linalg.solve in float64 of (M64 [+ diag(arm)]) x = rhs for rhs (n, 26) or (n, 26, r)."""
    M = np.asarray(M64, dtype=np.float64)
    if arm is not None:
        M = M + np.diag(np.asarray(arm, dtype=np.float64))[None]
    rhs = np.asarray(rhs, dtype=np.float64)
    return np.linalg.solve(M, rhs[:, :, None])[:, :, 0] if rhs.ndim == 2 else np.linalg.solve(M, rhs)


def regular_poses(hk, n, seed, min_cos=0.1):
    """The first n of HandKin.random_poses' draws whose base is not in gimbal lock: |cos q4| >= min_cos.  The base hinges 3-5 are
    Euler angles on massless links, so at q4 = +-pi/2 (joints 3 and 5 coaxial) M is exactly singular and the acceleration is not
    defined; the condition number of the d-scaled M grows like 10 / cos^2 q4 (1.8e9 at |q4 - pi/2| = 2e-4, at most 1.2e3 over 2000
    draws with |cos q4| >= 0.1, about 93 % of them), and with it the roundoff of ANY fp32 solve, so that 4 x the fp32 reference's
    figure stops being a bound there.  The residual E_res is not affected.
    Stated for any model: M is singular where the world axes of the hinges 3, 4, 5 are linearly dependent, and |det [a3 a4 a5]| is
    |cos q4| on the default model (axes e_x, e_y, e_z on coincident frames); a model with tilted axes has its lock elsewhere."""
    q = hk.random_poses(2 * n + 20, seed)
    g = hk.geom
    det = np.zeros(len(q))
    for i, x in enumerate(q.astype(np.float64)):
        R = g.fk(x)[1]
        det[i] = abs(np.linalg.det(np.stack([R[j] @ (g.jaxis[j] / np.linalg.norm(g.jaxis[j])) for j in (3, 4, 5)])))
    q = q[det >= min_cos]
    assert len(q) >= n
    return q[:n]


def targets(M64, b64, seed):
    """y uniform in +-10 and tau = float32(M64 y + b64): every joint's acceleration matters at its own scale."""
    y = np.random.default_rng(seed).uniform(-10.0, 10.0, b64.shape)
    return y, (np.einsum("nij,nj->ni", M64, y) + b64).astype(np.float32)


def err_qdd(x, x64, M64):
    """E_tau's form with the dual scaling d_j = sqrt(M64_jj): per pose max_j |x - x64|_j d_j over max_j |x64|_j d_j, the max over
    poses.  x (n, 26), or (n, 26, r): then every column is a pose of its own."""
    x, x64 = np.asarray(x, dtype=np.float64), np.asarray(x64, dtype=np.float64)
    d = np.sqrt(np.einsum("nii->ni", M64))
    if x.ndim == 3:
        d = d[:, :, None]
    num = (np.abs(x - x64) * d).max(1)
    den = (np.abs(x64) * d).max(1)
    return float((num / den).max())


def err_res(x, tau, M64, b64):
    """E_res: the residual M64 x + b64 against tau in invdyn_ref.err_tau's metric."""
    return ir.err_tau(np.einsum("nij,nj->ni", M64, np.asarray(x, dtype=np.float64)) + b64, np.asarray(tau, dtype=np.float64), M64)


def set_armature(ms, orc64, q_mid, seed=9):
    """Armatures of the size of M's own diagonal at the pose q_mid, times a factor in [0.5, 1.5] per joint (1e-6 .. 1e-4 on the
    finger joints, the hand's mass and inertia on the base joints), rounded to float32: leaving them out changes every
    acceleration by tens of per cent.  Sets ms.armature and returns the values as float64."""
    M, _ = orc64.mass_matrix(np.asarray(q_mid, dtype=np.float64), np.zeros(NJ))
    arm = (np.random.default_rng(seed).uniform(0.5, 1.5, NJ) * np.diag(M)).astype(np.float32)
    for j in range(NJ):
        ms.armature[j] = float(arm[j])
    return arm.astype(np.float64)
