"""Time the dynamics-derivative calls (dexsim_inverse_dynamics_derivatives, dexsim_forward_dynamics_derivatives) against two
yardsticks of the same run: k_kin_invdyn alone (one Newton-Euler walk: the unit the tangent passes are made of) and what a caller did
before these calls existed -- central differences, 52 back-to-back dexsim_inverse_dynamics launches on override rows (the launches
alone: perturbing the rows and forming the differences are left out, in the finite-difference route's favour).

    python scripts/dynderiv_timing.py [--num-envs 4096 16384] [--override-rows 65536] [--launches 100] [--tag TEXT] [--out FILE]
                                      [--readme FILE]

Cases per N: the inverse-dynamics derivatives with both outputs and with each alone, the forward-dynamics derivatives with both
outputs, the mass solve of one output's 26 rows (the forward route's last launch), the two yardsticks; once, on the last N, the same
on an override batch of `--override-rows` rows.  Per case: a warm-up block, then HIP events around blocks of 10 back-to-back
launches until `--launches` launches ran; the mean per launch is printed as one JSON line with its ratios to the two yardsticks of
the same row count.  DEXSIM_LIB_PATH selects another build of the library; --tag names it in the lines.  The figures in
profiles/dynamics_derivatives/README.md come from this script."""
import query_timing as qt
import torch

BLOCK = 10
WALK = "inverse dynamics (k_kin_invdyn)"
DIFFS = "finite differences: 52 inverse-dynamics launches"
COLUMNS = [("N", "num_envs"), ("case", "case"), ("rows", "rows"), ("µs", "us"), ("× inverse dynamics", "ratio_to_invdyn"),
           ("× finite differences", "ratio_to_differences")]


def main():
    args = qt.parser(launches=100, num_envs=[4096, 16384], override_rows=True, tag=True, readme=True).parse_args()
    from dexrobot_isaac_amd import _abi
    dev = qt.DEV
    NJ = _abi.NJ
    lines = []
    for n in args.num_envs:
        core, draws = qt.posed_core(n, speed=3.0)
        rnd = draws.sym

        def cases_for(k, tag, q=None, qd=None):
            acc, tau, out = rnd(10.0, k, NJ), rnd(1.0, k, NJ), torch.empty(k, NJ, device=dev)
            dq, dv = torch.empty(k, NJ, NJ, device=dev), torch.empty(k, NJ, NJ, device=dev)
            rhs = rnd(1.0, k, NJ, NJ)
            # the finite-difference route perturbs override rows: the state path's q and qd are read back for it
            oq = core.dof_state[:, :, 0].contiguous() if q is None else q
            ov = core.dof_state[:, :, 1].contiguous() if qd is None else qd

            def differences():
                for _ in range(2 * NJ):
                    core.inverse_dynamics(out, qdd=acc, q=oq, qd=ov)
            return [("inverse-dynamics derivatives, both" + tag, k, lambda: core.inverse_dynamics_derivatives(dq, dv, qdd=acc, q=q, qd=qd)),
                    ("inverse-dynamics derivatives, d/dq alone" + tag, k, lambda: core.inverse_dynamics_derivatives(dq, None, qdd=acc, q=q, qd=qd)),
                    ("inverse-dynamics derivatives, d/dqd alone" + tag, k, lambda: core.inverse_dynamics_derivatives(None, dv, qdd=acc, q=q, qd=qd)),
                    ("forward-dynamics derivatives, both" + tag, k, lambda: core.forward_dynamics_derivatives(out, dq, dv, tau=tau, q=q, qd=qd)),
                    ("mass solve, nrhs = 26, in place" + tag, k, lambda: core.mass_solve(rhs, rhs, q=q)),
                    (WALK + tag, k, lambda: core.inverse_dynamics(out, qdd=acc, q=q, qd=qd)),
                    (DIFFS + tag, k, differences)]
        cases = cases_for(n, "")
        if n == args.num_envs[-1]:
            k = args.override_rows
            cases += cases_for(k, ", overrides", q=draws.pose(k), qd=rnd(3.0, k, NJ))
        block = []
        for name, rows, fn in cases:
            block.append({"build": args.tag, "num_envs": n, "case": name, "rows": rows, "us": round(qt.measure(fn, args.launches, BLOCK), 1)})
        qt.add_ratio(block, "ratio_to_invdyn", WALK, 2)          # against the yardsticks of the same row count
        qt.add_ratio(block, "ratio_to_differences", DIFFS, 3)
        for x in block:
            qt.emit(x)
        lines += block
        core.close()
        del core, cases
        torch.cuda.empty_cache()
    qt.write(args, lines, COLUMNS)


if __name__ == "__main__":
    main()
