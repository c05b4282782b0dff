"""Reference for the fingertip inverse kinematics in control space (dexsim_solve_ik, include/dexsim.h): a plain numpy statement of
the iteration the header specifies, on tests/render_ref.HandGeometry.fk (its own forward kinematics from the header's joint-frame
formula) and site_parent / site_p / site_q of the model struct.  Every function takes `dtype`, so the SAME code runs in float64 and
float32: their difference is the roundoff figure the GPU tolerances rest on.  It shares no code with the engine; the coupling table
below is its own copy, as data.
"""
import numpy as np

from dexrobot_isaac_amd import _abi
from tests import render_ref as rr

NJ, NACT, NF = _abi.NJ, _abi.NACT, _abi.NFINGER

# control -> [(DOF, scale)] in the order of the 18 active targets; DOF 14 is driven by no control and stays 0
COUPLING = [
    [(0, 1.0)], [(1, 1.0)], [(2, 1.0)], [(3, 1.0)], [(4, 1.0)], [(5, 1.0)],
    [(6, 1.0)], [(7, 1.0)], [(8, 1.0), (9, 1.0)],
    [(10, 1.0), (18, 1.0), (22, 2.0)],
    [(11, 1.0)], [(12, 1.0), (13, 1.0)],
    [(15, 1.0)], [(16, 1.0), (17, 1.0)],
    [(19, 1.0)], [(20, 1.0), (21, 1.0)],
    [(23, 1.0)], [(24, 1.0), (25, 1.0)],
]
HELD_DOF = 14
FINGERS_FREE = sum(1 << c for c in range(6, NACT))
ALL_FREE = (1 << NACT) - 1


class HandIK:
    def __init__(self, ms, sc):
        self.geom = rr.HandGeometry(ms)
        self.site_parent = np.array(np.ctypeslib.as_array(ms.site_parent))
        self.site_p = np.array(np.ctypeslib.as_array(ms.site_p), dtype=np.float64)
        self.site_q = np.array(np.ctypeslib.as_array(ms.site_q), dtype=np.float64)
        self.lower = np.array(list(sc.active_lower), dtype=np.float32)          # what the engine was given
        self.upper = np.array(list(sc.active_upper), dtype=np.float32)
        self.C = np.zeros((NJ, NACT))
        for c, grp in enumerate(COUPLING):
            for d, s in grp:
                self.C[d, c] = s
        g = self.geom
        self.ancestors = []
        for j in range(NJ):
            a, p = [], j
            while p >= 0:
                a.append(p)
                p = g.parent(p)
            self.ancestors.append(a)

    # ---- the coupling (everything below is batched over rows: u (n, 18), q (n, 26))
    def q_of_u(self, u, dtype=np.float64):
        return (np.asarray(u, dtype=dtype) @ self.C.T.astype(dtype)).astype(dtype)

    def u0_of_q(self, q0, dtype=np.float64):
        first = [grp[0][0] for grp in COUPLING]
        return np.clip(np.asarray(q0, dtype=dtype)[..., first], self.lower.astype(dtype), self.upper.astype(dtype))

    # ---- kinematics in control space
    def fk(self, q, dtype=np.float64):
        """render_ref.HandGeometry.fk, the same formula joint by joint, for all rows of q (n, 26) at once: origins (n, 26, 3),
        rotations (n, 26, 3, 3).  tests/test_ik.py holds it against HandGeometry.fk row by row."""
        g = self.geom
        q = np.asarray(q, dtype=dtype)
        n = len(q)
        o = np.zeros((n, NJ, 3), dtype=dtype)
        R = np.zeros((n, NJ, 3, 3), dtype=dtype)
        I = np.eye(3, dtype=dtype)
        for j in range(NJ):
            p = g.parent(j)
            if p < 0:
                po = np.broadcast_to(g.spawn_pos.astype(dtype), (n, 3))
                pR = np.broadcast_to(rr.quat_to_mat(g.spawn_quat, dtype), (n, 3, 3))
            else:
                po, pR = o[:, p], R[:, p]
            oj = po + pR @ g.jpoff[j].astype(dtype)
            Rz = pR @ rr.quat_to_mat(g.jqoff[j], dtype)
            a = g.jaxis[j].astype(dtype)
            if g.jtype[j] == 0:
                oj = oj + q[:, j, None] * (Rz @ a)
                Rj = Rz
            else:
                c, s = np.cos(q[:, j])[:, None, None], np.sin(q[:, j])[:, None, None]
                K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=dtype)
                Rj = Rz @ (I * c + s * K + (1 - c) * np.outer(a, a)).astype(dtype)
            o[:, j], R[:, j] = oj, Rj
        return o, R

    def sites_of_q(self, q, sites, dtype=np.float64):
        """World positions (n, 5, 3) of the five sites (sites = 0 tips, 1 pads) and the joint frames."""
        o, R = self.fk(q, dtype)
        s0 = 6 if sites else 1
        par = [int(self.site_parent[s0 + f]) for f in range(NF)]
        p = np.stack([o[:, par[f]] + R[:, par[f]] @ self.site_p[s0 + f].astype(dtype) for f in range(NF)], axis=1)
        return p, o, R

    def site_pos(self, u, sites, dtype=np.float64):
        return self.sites_of_q(self.q_of_u(u, dtype), sites, dtype)[0]

    def hand_frame(self, u, dtype=np.float64):
        """Pose of site 0 (right_hand_base): origins (n, 3), rotations (n, 3, 3)."""
        o, R = self.fk(self.q_of_u(u, dtype), dtype)
        j = int(self.site_parent[0])
        return o[:, j] + R[:, j] @ self.site_p[0].astype(dtype), R[:, j] @ rr.quat_to_mat(self.site_q[0], dtype)

    def to_world(self, u0, targets, frame, dtype=np.float64):
        """Hand-frame targets (n, 5, 3) to world through site 0's pose at u0; world targets as they are."""
        t = np.asarray(targets, dtype=dtype)
        if frame == 1:
            hp, hR = self.hand_frame(u0, dtype)
            t = (hp[:, None, :] + np.einsum("nij,nfj->nfi", hR, t)).astype(dtype)
        return t

    def jacobian(self, u, sites, dtype=np.float64):
        """(n, 5, 3, 18): d p_f / d u_c, the joint columns folded through the coupling scales; also p (n, 5, 3)."""
        g = self.geom
        p, o, R = self.sites_of_q(self.q_of_u(u, dtype), sites, dtype)
        s0 = 6 if sites else 1
        J = np.zeros((len(p), NF, 3, NACT), dtype=dtype)
        for f in range(NF):
            anc = self.ancestors[self.site_parent[s0 + f]]
            for c, grp in enumerate(COUPLING):
                for d, s in grp:
                    if d not in anc:
                        continue
                    a = R[:, d] @ g.jaxis[d].astype(dtype)
                    col = a if g.jtype[d] == 0 else np.cross(a, p[:, f] - o[:, d])
                    J[:, f, :, c] += dtype(s) * col
        return J, p

    # ---- the iteration of the header, to the letter
    def solve(self, q0, targets, sites=0, frame=0, free_mask=FINGERS_FREE, iters=16, damping=1e-3, max_step=0.5,
              weight=(1, 1, 1, 1, 1), dtype=np.float64):
        """q0 (n, 26), targets (n, 5, 3) -> controls (n, 18), q_out (n, 26), residual (n, 5), all in `dtype`; rows are independent."""
        lo, hi = self.lower.astype(dtype), self.upper.astype(dtype)
        u = self.u0_of_q(q0, dtype)
        t = self.to_world(u, targets, frame, dtype)
        F = [c for c in range(NACT) if (free_mask >> c) & 1]
        w = np.asarray(weight, dtype=dtype)
        lam2 = dtype(damping) * dtype(damping)
        for _ in range(iters):
            J, p = self.jacobian(u, sites, dtype)
            A = np.zeros((len(u), len(F), len(F)), dtype=dtype)
            b = np.zeros((len(u), len(F)), dtype=dtype)
            for f in range(NF):                                                # fixed order f = 0..4
                Jf = J[:, f][:, :, F]
                A = A + w[f] * np.einsum("nki,nkj->nij", Jf, Jf)
                b = b + w[f] * np.einsum("nki,nk->ni", Jf, t[:, f] - p[:, f])
            A = (A + lam2 * np.eye(len(F), dtype=dtype)).astype(dtype)
            L = np.linalg.cholesky(A)
            y = np.linalg.solve(L, b[:, :, None])
            d = np.linalg.solve(np.swapaxes(L, 1, 2), y)[:, :, 0].astype(dtype)
            m = np.abs(d).max(1)
            s = np.where(m <= dtype(max_step), dtype(1), dtype(max_step) / np.maximum(m, dtype(1e-30))).astype(dtype)
            u = u.copy()
            u[:, F] = np.clip(u[:, F] + s[:, None] * d, lo[F], hi[F])
        res = np.sqrt(((t - self.site_pos(u, sites, dtype)) ** 2).sum(2)).astype(dtype)
        return u, self.q_of_u(u, dtype), res

    def residual64(self, u0, controls, targets, sites=0, frame=0):
        """|t_f - p_f(controls)| in float64, the hand-frame targets mapped through site 0's pose at u0: (n, 5)."""
        t = self.to_world(np.asarray(u0, dtype=np.float64), targets, frame)
        return np.sqrt(((t - self.site_pos(np.asarray(controls, dtype=np.float64), sites)) ** 2).sum(2))

    # ---- the poses of the tests
    def test_poses(self, n, seed, free_mask=FINGERS_FREE, pert=0.3, sites=0):
        """Start controls uniform in the active limits (base slides in +-0.3 m, base rotations in +-1 rad), float32; q0 = C u on the
        coupling manifold; targets = the float64 forward kinematics of the start controls perturbed by pert * U(-1, 1) *
        min(range, 1) on the free controls and clamped: reachable by construction.  Returns u_start (n, 18), q0 (n, 26),
        targets (n, 5, 3), all float32."""
        rng = np.random.default_rng(seed)
        lo, hi = self.lower.astype(np.float64), self.upper.astype(np.float64)
        lo_s, hi_s = lo.copy(), hi.copy()
        lo_s[0:3], hi_s[0:3] = np.maximum(lo[0:3], -0.3), np.minimum(hi[0:3], 0.3)
        lo_s[3:6], hi_s[3:6] = np.maximum(lo[3:6], -1.0), np.minimum(hi[3:6], 1.0)
        u = rng.uniform(lo_s, hi_s, (n, NACT)).astype(np.float32)
        u = np.clip(u, self.lower, self.upper)
        free = np.array([(free_mask >> c) & 1 for c in range(NACT)], dtype=np.float64)
        d = pert * rng.uniform(-1, 1, (n, NACT)) * np.minimum(hi - lo, 1.0) * free
        ug = np.clip(u.astype(np.float64) + d, lo, hi)
        tg = self.site_pos(ug, sites).astype(np.float32)
        q0 = self.q_of_u(u, np.float32)
        return u, q0, tg
