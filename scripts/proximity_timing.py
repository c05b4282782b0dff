"""Time the clearance query (dexsim_query_proximity).

    python scripts/proximity_timing.py [--rows 4096] [--launches 200] [--out FILE]

A BlindGrasping env of `--rows` envs after a few random control steps; the query runs on the state path (the envs' own q and box)
and through the q / box_pose override fed the same state.  Timing: HIP events around blocks of back-to-back calls, after a warm-up
block; `--launches` calls per figure.  One JSON line: microseconds per call for all three outputs on both paths and for each output
alone, and the bytes a call writes.  The figures in DESIGN.md ("Measurements: clearance queries") and profiles/proximity come from
this script."""
import query_timing as qt
import torch


def main():
    args = qt.parser(launches=200, rows=4096).parse_args()
    from dexrobot_isaac_amd import _abi, make_env
    dev = qt.DEV
    k = args.rows
    env = make_env("BlindGrasping", k, dev, dev, 0)
    env.reset()
    g = torch.Generator().manual_seed(0)
    for _ in range(5):
        env.step((2 * torch.rand(k, env.num_actions, generator=g) - 1).to(dev))
    core = env._core
    bufs = {"cap_env": torch.empty(k, _abi.NCAP, 2, 8, device=dev), "self_min": torch.empty(k, _abi.NPROX_GROUPS, 8, device=dev),
            "pair_dist": torch.empty(k, _abi.NPROX_PAIRS, device=dev)}
    q = env.dof_pos.clone().contiguous()
    box = core.root_state[:, 1, :7].clone().contiguous()
    cases = {"all_us": lambda: core.proximity(**bufs),
             "all_override_us": lambda: core.proximity(q=q, box_pose=box, **bufs)}
    for name, t in bufs.items():
        cases[name + "_us"] = (lambda name=name, t=t: core.proximity(**{name: t}))
    line = {"rows": k, "launches": args.launches, "bytes_written": sum(t.numel() * 4 for t in bufs.values())}
    for name, fn in cases.items():
        line[name] = round(qt.measure(fn, args.launches, 20), 1)
    state = {n: t.clone() for n, t in bufs.items()}
    core.proximity(q=q, box_pose=box, **bufs)
    torch.cuda.synchronize()
    line["override_equals_state_bitwise"] = all(torch.equal(state[n].view(torch.int32), bufs[n].view(torch.int32)) for n in bufs)
    line["min_box_distance_m"] = float(f"{float(bufs['cap_env'][:, :, 0, 0].min()):.4g}")
    line["min_self_distance_m"] = float(f"{float(bufs['pair_dist'].min()):.4g}")
    qt.emit(line)
    qt.write(args, [line])
    env.close()


if __name__ == "__main__":
    main()
