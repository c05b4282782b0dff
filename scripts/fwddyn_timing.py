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
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

BLOCK = 20
WALK = "inverse dynamics (k_kin_invdyn)"
BYHAND = "by hand: M + bias force + torch.linalg.solve"
COLS = (1, 6, 15, 26)


def time_block(fn, n):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1000.0          # us


def measure(fn, launches):
    fn()
    time_block(fn, BLOCK)                        # warm-up
    blocks = max(1, (launches + BLOCK - 1) // BLOCK)
    return sum(time_block(fn, BLOCK) for _ in range(blocks)) / (blocks * BLOCK)


def table(lines):
    out = ["| N | case | rows | µs | × inverse dynamics | × by hand |", "|---|---|---|---|---|---|"]
    for x in lines:
        out.append(f"| {x['num_envs']} | {x['case']} | {x['rows']} | {x['us']} | {x['ratio_to_invdyn']} | {x['ratio_to_by_hand']} |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--override-rows", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--tag", default="", help="names the build in the JSON lines")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--readme", default=None, help="write the table of this run (markdown) to this file")
    args = ap.parse_args()
    from dexrobot_isaac_amd import _abi
    from dexrobot_isaac_amd.config import build_sim_config, default_cfg
    from dexrobot_isaac_amd.core import DexSimCore
    dev = "cuda:0"
    NJ = _abi.NJ
    lines = []
    for n in args.num_envs:
        cfg = default_cfg("BlindGrasping")
        cfg["env"]["numEnvs"] = n
        sc, model = build_sim_config(cfg)
        core = DexSimCore(sc, model.to_struct(), dev)
        core.reset()
        g = torch.Generator(device=dev).manual_seed(0)
        lo = torch.tensor(list(core.model.lo), device=dev)
        hi = torch.tensor(list(core.model.hi), device=dev)
        rnd = lambda a, *s: a * (2 * torch.rand(*s, device=dev, generator=g) - 1)
        core.dof_state[:, :, 0] = lo + (hi - lo) * torch.rand(n, NJ, device=dev, generator=g)
        core.dof_state[:, :, 1] = rnd(3.0, n, NJ)
        core.set_dof_state_indexed(torch.arange(n, device=dev))

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
            cases += cases_for(k, ", overrides", q=lo + (hi - lo) * torch.rand(k, NJ, device=dev, generator=g), qd=rnd(3.0, k, NJ), cols=(6,))
        block = []
        for name, rows, fn in cases:
            block.append({"build": args.tag, "num_envs": n, "case": name, "rows": rows, "us": round(measure(fn, args.launches), 1)})
        for x in block:   # against the yardsticks of the same row count
            walk = next(y for y in block if y["case"].startswith(WALK) and y["rows"] == x["rows"])
            hand = next(y for y in block if y["case"].startswith(BYHAND) and y["rows"] == x["rows"])
            x["ratio_to_invdyn"] = round(x["us"] / walk["us"], 2)
            x["ratio_to_by_hand"] = round(x["us"] / hand["us"], 3)
            print(json.dumps(x), flush=True)
        lines += block
        core.close()
        del core, cases
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    if args.readme:
        os.makedirs(os.path.dirname(os.path.abspath(args.readme)), exist_ok=True)
        with open(args.readme, "w") as f:
            f.write(table(lines))


if __name__ == "__main__":
    main()
