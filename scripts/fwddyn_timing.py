"""Time the forward-dynamics / mass-solve kernel (dexsim_forward_dynamics, dexsim_mass_solve) against two yardsticks of the same
run: k_kin_invdyn alone (the shared walk: the floor of this design) and what a caller did before these calls existed --
dexsim_mass_matrix + the bias force of dexsim_inverse_dynamics + a batched torch.linalg.solve.

    python scripts/fwddyn_timing.py [--num-envs 4096 16384] [--override-rows 65536] [--launches 200] [--tag TEXT] [--out FILE]
                                    [--readme FILE]

Cases per N: forward dynamics with tau and free (tau NULL), the mass solve at nrhs = 1, 6, 15 and 26, the two yardsticks; once, on
the last N, forward dynamics, the mass solve at nrhs = 6 and the yardsticks on an override batch of `--override-rows` rows.  Per
case: a warm-up block, then HIP events around blocks of 20 back-to-back launches until `--launches` launches ran; the mean per
launch is printed as one JSON line with its ratios to the two yardsticks of the same row count.  DEXSIM_LIB_PATH selects another
build of the library (the FD_COLS variants of dexsim_fwddyn.hip.inc); --tag names it in the lines.  The figures in DESIGN.md
("Measurements: forward dynamics") and profiles/forward_dynamics/README.md come from this script."""
import query_timing as qt
import torch

BLOCK = 20
WALK = "inverse dynamics (k_kin_invdyn)"
BYHAND = "by hand: M + bias force + torch.linalg.solve"
COLS = (1, 6, 15, 26)
COLUMNS = [("N", "num_envs"), ("case", "case"), ("rows", "rows"), ("µs", "us"), ("× inverse dynamics", "ratio_to_invdyn"),
           ("× by hand", "ratio_to_by_hand")]


def main():
    args = qt.parser(launches=200, num_envs=[4096, 16384], override_rows=True, tag=True, readme=True).parse_args()
    from dexrobot_isaac_amd import _abi
    dev = qt.DEV
    NJ = _abi.NJ
    lines = []
    for n in args.num_envs:
        core, draws = qt.posed_core(n, speed=3.0)
        rnd = draws.sym

        def cases_for(k, tag, q=None, qd=None, cols=COLS):
            tau, out = rnd(1.0, k, NJ), torch.empty(k, NJ, device=dev)
            M, b = torch.empty(k, NJ, NJ, device=dev), torch.empty(k, NJ, device=dev)

            def by_hand():
                core.mass_matrix(mass=M, q=q)
                core.inverse_dynamics(b, q=q, qd=qd)
                return torch.linalg.solve(M, (tau - b).unsqueeze(-1))
            cs = [("forward dynamics, tau" + tag, k, lambda: core.forward_dynamics(out, tau=tau, q=q, qd=qd)),
                  ("forward dynamics, free (tau NULL)" + tag, k, lambda: core.forward_dynamics(out, q=q, qd=qd))]
            for r in cols:
                rhs, x = rnd(1.0, k, r, NJ), torch.empty(k, r, NJ, device=dev)
                cs.append((f"mass solve, nrhs = {r}" + tag, k, lambda rhs=rhs, x=x: core.mass_solve(x, rhs, q=q)))
            cs.append((WALK + tag, k, lambda: core.inverse_dynamics(b, qdd=tau, q=q, qd=qd)))
            cs.append((BYHAND + tag, k, by_hand))
            return cs
        cases = cases_for(n, "")
        if n == args.num_envs[-1]:
            k = args.override_rows
            cases += cases_for(k, ", overrides", q=draws.pose(k), qd=rnd(3.0, k, NJ), cols=(6,))
        block = []
        for name, rows, fn in cases:
            block.append({"build": args.tag, "num_envs": n, "case": name, "rows": rows, "us": round(qt.measure(fn, args.launches, BLOCK), 1)})
        qt.add_ratio(block, "ratio_to_invdyn", WALK, 2)          # against the yardsticks of the same row count
        qt.add_ratio(block, "ratio_to_by_hand", BYHAND, 3)
        for x in block:
            qt.emit(x)
        lines += block
        core.close()
        del core, cases
        torch.cuda.empty_cache()
    qt.write(args, lines, COLUMNS)


if __name__ == "__main__":
    main()
