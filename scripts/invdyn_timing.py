"""Time the inverse-dynamics / bias-acceleration kernels (dexsim_inverse_dynamics, dexsim_body_bias_accel) against their write
floor and against k_kin_mass, whose phase A is the comparable chain walk.

    python scripts/invdyn_timing.py [--num-envs 4096 16384] [--override-rows 65536] [--launches 200] [--out FILE] [--readme FILE]

Cases per N: (a) tau with qdd and gravity, (b) the bias force (qdd NULL), (c) Jdot qd of the 6 bodies right_hand_base + the five
*_tip, (d) Jdot qd of all 37 bodies, (e) the yardstick: M + gravity force of dexsim_mass_matrix; once, on the last N: (f) tau and
(g) M + gravity on an override batch of `--override-rows` rows.  Per case: a warm-up block, then HIP events around blocks of 20
back-to-back launches until `--launches` launches ran; the mean per launch is printed as one JSON line next to the floor = bytes
written / 8 TB/s (HBM3E peak of the MI355X), their ratio and the ratio to the yardstick of the same N.  The outputs of a case are
written once per launch and never read back; the inputs (q, qd, qdd: 312 B per row) are of the size of tau (104 B per row), so
for tau the floor of the whole traffic is up to 4 x the write floor stated.  The figures in DESIGN.md ("Measurements: inverse
dynamics") and profiles/inverse_dynamics/README.md come from this script."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

BLOCK = 20
PEAK_BPS = 8.0e12
YARDSTICK = "mass matrix + gravity"


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
    out = ["| N | case | rows | MB written | µs | floor µs | ratio to floor | ratio to M + gravity |", "|---|---|---|---|---|---|---|---|"]
    for x in lines:
        out.append(f"| {x['num_envs']} | {x['case']} | {x['rows']} | {x['MB_written']} | {x['us']} | {x['floor_us_at_8TBps']} | {x['ratio']} "
                   f"| {x['ratio_to_mass_matrix']} |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--override-rows", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--readme", default=None, help="write the table of this run (markdown) to this file")
    args = ap.parse_args()
    from dexrobot_isaac_amd import _abi
    from dexrobot_isaac_amd.config import build_sim_config, default_cfg
    from dexrobot_isaac_amd.core import DexSimCore
    from dexrobot_isaac_amd.hand_model import BODY_NAMES, FINGERTIP_BODY_NAMES
    dev = "cuda:0"
    NJ, NB = _abi.NJ, _abi.NUM_HAND_BODIES
    six = [BODY_NAMES.index(n) for n in ["right_hand_base"] + FINGERTIP_BODY_NAMES]
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
        rates = lambda rows, a: a * (2 * torch.rand(rows, NJ, device=dev, generator=g) - 1)
        core.dof_state[:, :, 0] = lo + (hi - lo) * torch.rand(n, NJ, device=dev, generator=g)
        core.dof_state[:, :, 1] = rates(n, 3.0)
        core.set_dof_state_indexed(torch.arange(n, device=dev))
        qdd = rates(n, 10.0)
        tau = torch.empty(n, NJ, device=dev)
        a6, a37 = torch.empty(n, 6, 6, device=dev), torch.empty(n, NB, 6, device=dev)
        M, grav = torch.empty(n, NJ, NJ, device=dev), torch.empty(n, NJ, device=dev)
        cases = [
            ("tau = M qdd + c + g", n, tau.numel() * 4, lambda: core.inverse_dynamics(tau, qdd=qdd)),
            ("bias force c + g (qdd NULL)", n, tau.numel() * 4, lambda: core.inverse_dynamics(tau)),
            ("Jdot qd, 6 bodies (right_hand_base + 5 tips)", n, a6.numel() * 4, lambda: core.body_bias_accel(a6, bodies=six)),
            ("Jdot qd, all 37 bodies", n, a37.numel() * 4, lambda: core.body_bias_accel(a37)),
            (YARDSTICK, n, (M.numel() + grav.numel()) * 4, lambda: core.mass_matrix(mass=M, gravity=grav)),
        ]
        if n == args.num_envs[-1]:
            k = args.override_rows
            qo = lo + (hi - lo) * torch.rand(k, NJ, device=dev, generator=g)
            vo, ao = rates(k, 3.0), rates(k, 10.0)
            to = torch.empty(k, NJ, device=dev)
            Mo, go = torch.empty(k, NJ, NJ, device=dev), torch.empty(k, NJ, device=dev)
            cases.append(("tau = M qdd + c + g, overrides", k, to.numel() * 4, lambda: core.inverse_dynamics(to, qdd=ao, q=qo, qd=vo)))
            cases.append((YARDSTICK + ", q override", k, (Mo.numel() + go.numel()) * 4, lambda: core.mass_matrix(mass=Mo, gravity=go, q=qo)))
        block = []
        for name, rows, nbytes, fn in cases:
            us = measure(fn, args.launches)
            floor = nbytes / PEAK_BPS * 1e6
            block.append({"num_envs": n, "case": name, "rows": rows, "MB_written": round(nbytes / 1e6, 2), "us": round(us, 1),
                          "floor_us_at_8TBps": round(floor, 2), "ratio": round(us / floor, 1)})
        for x in block:   # against the yardstick of the same row count
            ref = next(y for y in block if y["case"].startswith(YARDSTICK) and y["rows"] == x["rows"])
            x["ratio_to_mass_matrix"] = round(x["us"] / ref["us"], 2)
            print(json.dumps(x), flush=True)
        lines += block
        core.close()
        del core, tau, a6, a37, M, grav
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
