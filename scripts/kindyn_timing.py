"""Time the Jacobian / mass-matrix kernels (dexsim_body_jacobian, dexsim_mass_matrix) against their write floor.

    python scripts/kindyn_timing.py [--num-envs 4096 16384] [--override-rows 65536] [--launches 200] [--out FILE]

Cases per N: (a) Jacobians of the 6 bodies right_hand_base + the five *_tip, (b) Jacobians of all 37 bodies, (c) M + gravity force;
once, on the last N: (d) M + gravity on a q-override batch of `--override-rows` rows.  Per case: a warm-up block, then HIP events
around blocks of 20 back-to-back launches until `--launches` launches ran; the mean per launch is printed as one JSON line next to
the floor = bytes written / 8 TB/s (HBM3E peak of the MI355X) and their ratio.  The outputs of a case are written once per launch
and never read back, so bytes written is the whole traffic the shape requires (q is 104 B per row against >= 2.8 KB of output).
The figures in DESIGN.md ("Measurements: Jacobians, mass matrix, gravity force") and profiles/kindyn/README.md come from this script."""
import query_timing as qt
import torch

BLOCK = 20
PEAK_BPS = 8.0e12


def main():
    args = qt.parser(launches=200, num_envs=[4096, 16384], override_rows=True).parse_args()
    from dexrobot_isaac_amd import _abi
    from dexrobot_isaac_amd.hand_model import BODY_NAMES, FINGERTIP_BODY_NAMES
    dev = qt.DEV
    NJ = _abi.NJ
    six = [BODY_NAMES.index(n) for n in ["right_hand_base"] + FINGERTIP_BODY_NAMES]
    lines = []
    for n in args.num_envs:
        core, draws = qt.posed_core(n)
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
            qo = draws.pose(k)
            Mo, go = torch.empty(k, NJ, NJ, device=dev), torch.empty(k, NJ, device=dev)
            cases.append(("mass matrix + gravity, q override", k, (Mo.numel() + go.numel()) * 4,
                          lambda: core.mass_matrix(mass=Mo, gravity=go, q=qo)))
        for name, rows, nbytes, fn in cases:
            us = qt.measure(fn, args.launches, BLOCK)
            floor = nbytes / PEAK_BPS * 1e6
            line = {"num_envs": n, "case": name, "rows": rows, "MB_written": round(nbytes / 1e6, 2), "us": round(us, 1),
                    "floor_us_at_8TBps": round(floor, 1), "ratio": round(us / floor, 2), "GBps_written": round(nbytes / us / 1e3, 1)}
            qt.emit(line)
            lines.append(line)
        core.close()
        del core, j6, j37, M, grav
        torch.cuda.empty_cache()
    qt.write(args, lines)


if __name__ == "__main__":
    main()
