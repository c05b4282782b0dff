"""Time the Jacobian / mass-matrix kernels (dexsim_body_jacobian, dexsim_mass_matrix) against their write floor.

    python scripts/kindyn_timing.py [--num-envs 4096 16384] [--override-rows 65536] [--launches 200] [--out FILE]

Cases per N: (a) Jacobians of the 6 bodies right_hand_base + the five *_tip, (b) Jacobians of all 37 bodies, (c) M + gravity force;
once, on the last N: (d) M + gravity on a q-override batch of `--override-rows` rows.  Per case: a warm-up block, then HIP events
around blocks of 20 back-to-back launches until `--launches` launches ran; the mean per launch is printed as one JSON line next to
the floor = bytes written / 8 TB/s (HBM3E peak of the MI355X) and their ratio.  The outputs of a case are written once per launch
and never read back, so bytes written is the whole traffic the shape requires (q is 104 B per row against >= 2.8 KB of output).
The figures in DESIGN.md ("Measurements: Jacobians, mass matrix, gravity force") and profiles/kindyn/README.md come from this script."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

BLOCK = 20
PEAK_BPS = 8.0e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--override-rows", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from dexrobot_isaac_amd import _abi
    from dexrobot_isaac_amd.config import build_sim_config, default_cfg
    from dexrobot_isaac_amd.core import DexSimCore
    from dexrobot_isaac_amd.hand_model import BODY_NAMES, FINGERTIP_BODY_NAMES
    dev = "cuda:0"
    NJ = _abi.NJ
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
        core.dof_state[:, :, 0] = lo + (hi - lo) * torch.rand(n, NJ, device=dev, generator=g)
        core.set_dof_state_indexed(torch.arange(n, device=dev))
        j6 = torch.empty(n, 6, 6, NJ, device=dev)
        j37 = torch.empty(n, _abi.NUM_HAND_BODIES, 6, NJ, device=dev)
        M, grav = torch.empty(n, NJ, NJ, device=dev), torch.empty(n, NJ, device=dev)
        cases = [
            ("jacobian, 6 bodies (right_hand_base + 5 tips)", n, j6.numel() * 4, lambda: core.body_jacobian(j6, bodies=six)),
            ("jacobian, all 37 bodies", n, j37.numel() * 4, lambda: core.body_jacobian(j37)),
            ("mass matrix + gravity", n, (M.numel() + grav.numel()) * 4, lambda: core.mass_matrix(mass=M, gravity=grav)),
        ]
        if n == args.num_envs[-1]:
            k = args.override_rows
            qo = lo + (hi - lo) * torch.rand(k, NJ, device=dev, generator=g)
            Mo, go = torch.empty(k, NJ, NJ, device=dev), torch.empty(k, NJ, device=dev)
            cases.append(("mass matrix + gravity, q override", k, (Mo.numel() + go.numel()) * 4,
                          lambda: core.mass_matrix(mass=Mo, gravity=go, q=qo)))
        for name, rows, nbytes, fn in cases:
            us = measure(fn, args.launches)
            floor = nbytes / PEAK_BPS * 1e6
            line = {"num_envs": n, "case": name, "rows": rows, "MB_written": round(nbytes / 1e6, 2), "us": round(us, 1),
                    "floor_us_at_8TBps": round(floor, 1), "ratio": round(us / floor, 2), "GBps_written": round(nbytes / us / 1e3, 1)}
            print(json.dumps(line), flush=True)
            lines.append(line)
        core.close()
        del core, j6, j37, M, grav
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
