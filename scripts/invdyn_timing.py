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
import query_timing as qt
import torch

BLOCK = 20
PEAK_BPS = 8.0e12
YARDSTICK = "mass matrix + gravity"
COLUMNS = [("N", "num_envs"), ("case", "case"), ("rows", "rows"), ("MB written", "MB_written"), ("µs", "us"),
           ("floor µs", "floor_us_at_8TBps"), ("ratio to floor", "ratio"), ("ratio to M + gravity", "ratio_to_mass_matrix")]


def main():
    args = qt.parser(launches=200, num_envs=[4096, 16384], override_rows=True, readme=True).parse_args()
    from dexrobot_isaac_amd import _abi
    from dexrobot_isaac_amd.hand_model import BODY_NAMES, FINGERTIP_BODY_NAMES
    dev = qt.DEV
    NJ, NB = _abi.NJ, _abi.NUM_HAND_BODIES
    six = [BODY_NAMES.index(n) for n in ["right_hand_base"] + FINGERTIP_BODY_NAMES]
    lines = []
    for n in args.num_envs:
        core, draws = qt.posed_core(n, speed=3.0)
        qdd = draws.sym(10.0, n, NJ)
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
            qo = draws.pose(k)
            vo, ao = draws.sym(3.0, k, NJ), draws.sym(10.0, k, NJ)
            to = torch.empty(k, NJ, device=dev)
            Mo, go = torch.empty(k, NJ, NJ, device=dev), torch.empty(k, NJ, device=dev)
            cases.append(("tau = M qdd + c + g, overrides", k, to.numel() * 4, lambda: core.inverse_dynamics(to, qdd=ao, q=qo, qd=vo)))
            cases.append((YARDSTICK + ", q override", k, (Mo.numel() + go.numel()) * 4, lambda: core.mass_matrix(mass=Mo, gravity=go, q=qo)))
        block = []
        for name, rows, nbytes, fn in cases:
            us = qt.measure(fn, args.launches, BLOCK)
            floor = nbytes / PEAK_BPS * 1e6
            block.append({"num_envs": n, "case": name, "rows": rows, "MB_written": round(nbytes / 1e6, 2), "us": round(us, 1),
                          "floor_us_at_8TBps": round(floor, 2), "ratio": round(us / floor, 1)})
        qt.add_ratio(block, "ratio_to_mass_matrix", YARDSTICK, 2)   # against the yardstick of the same row count
        for x in block:
            qt.emit(x)
        lines += block
        core.close()
        del core, tau, a6, a37, M, grav
        torch.cuda.empty_cache()
    qt.write(args, lines, COLUMNS)


if __name__ == "__main__":
    main()
