"""Time the forward-kinematics kernel (dexsim_forward_kinematics) against its write floor and against dexsim_refresh_body_states,
the engine's own forward kinematics of the envs' state into the bound API tensors.

    python scripts/fk_timing.py [--num-envs 4096] [--override-rows 65536] [--launches 200] [--out FILE] [--readme FILE]

Cases per N, on the envs' state, and once more on a (q, qd) override batch of `--override-rows` rows: (a) body_states of all 37
bodies, (b) site_poses only, (c) centroid only, (d) all three in one call; per N the yardstick (e): one dexsim_refresh_body_states
launch, which writes rigid_body_states and contact_forces_all of every body (the box included), dof_state and the root states.
Per case: a warm-up block, then HIP events around blocks of 20 back-to-back launches until `--launches` launches ran; the mean per
launch is printed as one JSON line next to the floor = bytes written / 8 TB/s (HBM3E peak of the MI355X), their ratio and, on the
state path, the ratio to the yardstick of the same N (the yardstick has no overrides, so the override lines carry none).  The
outputs of a case are written once per launch and never read back.  The figures in DESIGN.md ("Measurements: forward kinematics")
and profiles/forward_kinematics/README.md come from this script."""
import query_timing as qt
import torch

BLOCK = 20
PEAK_BPS = 8.0e12
YARDSTICK = "refresh_body_states"
COLUMNS = [("N", "num_envs"), ("case", "case"), ("rows", "rows"), ("MB written", "MB_written"), ("µs", "us"),
           ("floor µs", "floor_us_at_8TBps"), ("ratio to floor", "ratio"), ("ratio to refresh_body_states", "ratio_to_refresh")]


def main():
    args = qt.parser(launches=200, num_envs=[4096], override_rows=True, readme=True).parse_args()
    from dexrobot_isaac_amd import _abi
    dev = qt.DEV
    NJ, NB, NS = _abi.NJ, _abi.NUM_HAND_BODIES, _abi.NSITE
    lines = []
    for n in args.num_envs:
        core, draws = qt.posed_core(n, speed=3.0)

        def cases_of(k, tag, **rows):
            body, site, cen = torch.empty(k, NB, 13, device=dev), torch.empty(k, NS, 7, device=dev), torch.empty(k, 8, device=dev)
            fk = core.forward_kinematics
            return [("body_states, all 37 bodies" + tag, k, body.numel() * 4, lambda: fk(body_states=body, **rows)),
                    ("site_poses only" + tag, k, site.numel() * 4, lambda: fk(site_poses=site, **rows)),
                    ("centroid only" + tag, k, cen.numel() * 4, lambda: fk(centroid=cen, **rows)),
                    ("all three in one call" + tag, k, (body.numel() + site.numel() + cen.numel()) * 4,
                     lambda: fk(body_states=body, site_poses=site, centroid=cen, **rows))]
        cases = cases_of(n, "")
        published = sum(t.numel() * t.element_size() for t in (core.rigid_body_states, core.contact_forces_all, core.dof_state, core.root_state))
        cases.append((YARDSTICK, n, published, core.refresh_body_states))
        if n == args.num_envs[-1]:
            k = args.override_rows
            cases += cases_of(k, ", q and qd overrides", q=draws.pose(k), qd=draws.sym(3.0, k, NJ))
        block = []
        for name, rows, nbytes, fn in cases:
            us = qt.measure(fn, args.launches, BLOCK)
            floor = nbytes / PEAK_BPS * 1e6
            block.append({"num_envs": n, "case": name, "rows": rows, "MB_written": round(nbytes / 1e6, 2), "us": round(us, 1),
                          "floor_us_at_8TBps": round(floor, 2), "ratio": round(us / floor, 1), "block": BLOCK, "launches": args.launches})
        state = [x for x in block if x["rows"] == n]
        qt.add_ratio(state, "ratio_to_refresh", YARDSTICK, 2)   # the yardstick has no overrides: the override lines carry no ratio
        for x in block:
            x.setdefault("ratio_to_refresh", "")
            qt.emit(x)
        lines += block
        core.close()
        del core
        torch.cuda.empty_cache()
    qt.write(args, lines, COLUMNS)


if __name__ == "__main__":
    main()
