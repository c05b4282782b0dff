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
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

BLOCK = 10
WALK = "inverse dynamics (k_kin_invdyn)"
DIFFS = "finite differences: 52 inverse-dynamics launches"


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
    out = ["| N | case | rows | µs | × inverse dynamics | × finite differences |", "|---|---|---|---|---|---|"]
    for x in lines:
        out.append(f"| {x['num_envs']} | {x['case']} | {x['rows']} | {x['us']} | {x['ratio_to_invdyn']} | {x['ratio_to_differences']} |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--override-rows", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=100)
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
            cases += cases_for(k, ", overrides", q=lo + (hi - lo) * torch.rand(k, NJ, device=dev, generator=g), qd=rnd(3.0, k, NJ))
        block = []
        for name, rows, fn in cases:
            block.append({"build": args.tag, "num_envs": n, "case": name, "rows": rows, "us": round(measure(fn, args.launches), 1)})
        for x in block:   # against the yardsticks of the same row count
            walk = next(y for y in block if y["case"].startswith(WALK) and y["rows"] == x["rows"])
            diffs = next(y for y in block if y["case"].startswith(DIFFS) and y["rows"] == x["rows"])
            x["ratio_to_invdyn"] = round(x["us"] / walk["us"], 2)
            x["ratio_to_differences"] = round(x["us"] / diffs["us"], 3)
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
