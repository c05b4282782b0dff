"""Time the fingertip IK kernel (dexsim_solve_ik) against the same iteration composed from env.get_jacobian plus torch ops.

    python scripts/ik_timing.py [--rows 4096] [--iters 16] [--launches 100] [--out FILE]

Both sides run the iteration of include/dexsim.h ("fingertip inverse kinematics in control space") with the finger controls free,
lambda = 1e-3, max_step = 0.5, from the same start poses towards the same reachable targets:
  kernel    one DexSimCore.solve_ik launch for all `--iters` iterations;
  composed  per iteration: q = C u, env.get_jacobian(bodies=<5 tips>, q=q) (the tip bodies' origins are the tip sites), the 26 DOF
            columns folded through the coupling matrix, a batched forward kinematics of the sites in torch (the project has no
            device service for p(q) at an arbitrary q), A and b by batched products, torch.linalg.cholesky + cholesky_solve, the step
            limit and the clamp -- everything on the device, no host synchronisation inside the loop.
Timing: HIP events around blocks of back-to-back solves, after a warm-up block; `--launches` solves per figure.  One JSON line:
both times, their ratio, the share of rows the kernel brings within 0.1 mm on every finger in `--iters` iterations, the median of
the rows' worst residual and the largest difference of the two results on those rows.  The figures in DESIGN.md ("Measurements:
fingertip IK") and profiles/ik come from this script."""
import numpy as np
import query_timing as qt
import torch


def quat_to_mat(q):
    x, y, z, w = [float(v) for v in np.asarray(q, dtype=np.float64) / np.linalg.norm(q)]
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]


class TorchSites:
    """Fingertip site positions p(q) (k, 5, 3) in torch: the base chain joint by joint, the five finger chains side by side."""

    def __init__(self, ms, dev):
        T = lambda a: torch.tensor(np.array(a, dtype=np.float64), dtype=torch.float32, device=dev)
        self.spawn_p, self.spawn_R = T(list(ms.spawn_pos)), T(quat_to_mat(list(ms.spawn_quat)))
        self.poff = T([list(ms.jpoff[j]) for j in range(26)])
        self.Rq = T([quat_to_mat(list(ms.jqoff[j])) for j in range(26)])
        self.ax = T([list(ms.jaxis[j]) for j in range(26)])
        a = self.ax
        z = torch.zeros(26, device=dev)
        self.K = torch.stack([torch.stack([z, -a[:, 2], a[:, 1]], 1), torch.stack([a[:, 2], z, -a[:, 0]], 1),
                              torch.stack([-a[:, 1], a[:, 0], z], 1)], 1)                       # (26, 3, 3)
        self.aa = a[:, :, None] * a[:, None, :]
        self.I = torch.eye(3, device=dev)
        self.site_p = T([list(ms.site_p[1 + f]) for f in range(5)])
        self.fj = torch.arange(5, device=dev) * 4 + 6

    def __call__(self, q):
        k = q.shape[0]
        o, R = self.spawn_p.expand(k, 3), self.spawn_R.expand(k, 3, 3)
        for j in range(6):
            o = o + R @ self.poff[j]
            Rz = R @ self.Rq[j]
            if j < 3:
                o = o + q[:, j, None] * (Rz @ self.ax[j])
                R = Rz
            else:
                c, s = torch.cos(q[:, j])[:, None, None], torch.sin(q[:, j])[:, None, None]
                R = Rz @ (self.I * c + s * self.K[j] + (1 - c) * self.aa[j])
        o, R = o[:, None, :].expand(k, 5, 3), R[:, None].expand(k, 5, 3, 3)
        for l in range(4):
            j = self.fj + l
            o = o + (R @ self.poff[j][None, :, :, None])[..., 0]
            Rz = R @ self.Rq[j]
            c, s = torch.cos(q[:, j])[..., None, None], torch.sin(q[:, j])[..., None, None]
            R = Rz @ (self.I * c + s * self.K[j] + (1 - c) * self.aa[j])
        return o + (R @ self.site_p[None, :, :, None])[..., 0]


def main():
    ap = qt.parser(launches=100, rows=4096)
    ap.add_argument("--iters", type=int, default=16)
    args = ap.parse_args()
    from dexrobot_isaac_amd import _abi, make_env
    from dexrobot_isaac_amd.config import FINGER_COUPLING_MAP
    from dexrobot_isaac_amd.hand_model import FINGERTIP_BODY_NAMES
    dev = qt.DEV
    k, NJ, NACT = args.rows, _abi.NJ, _abi.NACT
    env = make_env("BlindGrasping", k, dev, dev, 0)
    env.reset()
    core, ms = env._core, env._model_struct
    names = env.model.dof_names
    Cm = torch.zeros(NJ, NACT, device=dev)
    for c in range(6):
        Cm[c, c] = 1.0
    for c, grp in FINGER_COUPLING_MAP.items():
        for jn, sc in grp:
            Cm[names.index(jn), 6 + c] = sc
    lo, hi = env.action_processor.active_lower_limits, env.action_processor.active_upper_limits
    g = torch.Generator(device=dev).manual_seed(0)
    span = torch.minimum(hi - lo, torch.ones_like(hi))
    blo, bhi = lo.clone(), hi.clone()
    blo[:3], bhi[:3], blo[3:6], bhi[3:6] = -0.3, 0.3, -1.0, 1.0
    u0 = blo + (bhi - blo) * torch.rand(k, NACT, device=dev, generator=g)
    free = torch.zeros(NACT, device=dev)
    free[6:] = 1.0
    ug = torch.clamp(u0 + 0.3 * (2 * torch.rand(k, NACT, device=dev, generator=g) - 1) * span * free, lo, hi)
    sites = TorchSites(ms, dev)
    q0 = (u0 @ Cm.T).contiguous()
    targets = sites(ug @ Cm.T).contiguous()
    lam2, max_step, F = 1e-3 ** 2, 0.5, slice(6, NACT)
    eye = torch.eye(NACT - 6, device=dev)

    controls = torch.empty(k, NACT, device=dev)
    resid = torch.empty(k, 5, device=dev)

    def kernel():
        core.solve_ik(targets, controls, q=q0, iters=args.iters, damping=1e-3, max_step=max_step, residual=resid)

    jac = torch.empty(k, 5, 6, NJ, device=dev)
    result = {}

    def composed():
        u = u0.clone()
        for _ in range(args.iters):
            q = u @ Cm.T
            env.get_jacobian(bodies=FINGERTIP_BODY_NAMES, q=q, out=jac)
            J = (jac[:, :, 0:3, :] @ Cm)[..., F]                                  # (k, 5, 3, 12)
            e = targets - sites(q)
            A = torch.einsum("nfki,nfkj->nij", J, J) + lam2 * eye
            b = torch.einsum("nfki,nfk->ni", J, e)
            d = torch.cholesky_solve(b[:, :, None], torch.linalg.cholesky(A))[:, :, 0]
            m = d.abs().amax(1, keepdim=True)
            s = torch.where(m > max_step, max_step / m, torch.ones_like(m))
            u[:, F] = torch.clamp(u[:, F] + s * d, lo[F], hi[F])
        result["u"] = u

    kernel()
    composed()
    torch.cuda.synchronize()
    worst = resid.amax(1)                                                       # per row, over the five fingers
    conv = worst <= 1e-4
    diff = float((result["u"] - controls)[conv].abs().max())
    t_kernel = qt.measure(kernel, args.launches, 20)
    t_comp = qt.measure(composed, args.launches, 5)
    line = {"rows": k, "iters": args.iters, "free": "fingers", "kernel_us": round(t_kernel, 1), "composed_us": round(t_comp, 1),
            "ratio": round(t_comp / t_kernel, 1), "kernel_us_per_iteration": round(t_kernel / args.iters, 2),
            "rows_within_0.1mm": round(float(conv.float().mean()), 4), "median_residual_m": float(f"{float(worst.median()):.3g}"),
            "max_abs_diff_of_controls_on_those_rows": float(f"{diff:.3g}"), "launches": args.launches}
    qt.emit(line)
    qt.write(args, [line])
    env.close()


if __name__ == "__main__":
    main()
