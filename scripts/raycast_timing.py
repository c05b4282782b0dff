"""Time the range sensors (dexsim_raycast) against what a user would do without them: one camera image per env.

    python scripts/raycast_timing.py [--rows 4096] [--override-rows 65536] [--launches 200] [--out FILE] [--readme FILE]

A BlindGrasping env of `--rows` envs after a few random control steps.  The ray sets are R = 16, 64 and 1024 rays on the frames a
sensor suite uses: a quarter on the palm frame, a quarter on the distal joint frames, a quarter on the world frame, the rest spread
over all 26 joints; directions uniform on the sphere, origins within 3 cm of the frame (1 m above the ground for the world frame).
Cases: the state path (the envs' own q and box) with both outputs, with `dist` alone and with `hits` alone, and the q / box_pose
override on `--override-rows` rows with R = 16.  The yardstick comes from the same run: dexsim_render of one W x H = R depth image per
env from a world camera, scene pass included.  The write floor is the bytes a call writes at 8 TB/s.  Timing: HIP events around
blocks of 20 back-to-back calls, after a warm-up block, `--launches` calls per figure; the whole list is measured twice (run 0, 1).
One JSON line per case and run.  The figures of profiles/ray_sensors come from this script."""
import math

import query_timing as qt
import torch

HBM_BYTES_PER_US = 8e6   # 8 TB/s


def ray_set(R, seed=0):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(R, 3, generator=g)
    o = 0.03 * (2 * torch.rand(R, 3, generator=g) - 1)
    parent = []
    for i in range(R):
        m = i % 4
        parent.append(5 if m == 0 else 9 + 4 * ((i // 4) % 5) if m == 1 else -1 if m == 2 else (i // 4) % 26)
    parent = torch.tensor(parent)
    o[parent < 0, 2] += 1.0
    order = torch.sort(parent, stable=True).indices
    return torch.cat([o, d], 1)[order].contiguous().to(qt.DEV), parent[order].tolist()


def image_shape(R):
    w = 2 ** math.ceil(math.log2(R) / 2)
    return w, R // w


def main():
    ap = qt.parser(launches=200, rows=4096, override_rows=True, readme=True)
    args = ap.parse_args()
    from dexrobot_isaac_amd import _abi, make_env
    dev = qt.DEV
    k = args.rows
    env = make_env("BlindGrasping", k, dev, dev, 0)
    env.reset()
    g = torch.Generator().manual_seed(0)
    for _ in range(5):
        env.step((2 * torch.rand(k, env.num_actions, generator=g) - 1).to(dev))
    core = env._core
    ko = args.override_rows
    reps = (ko + k - 1) // k
    qo = env.dof_pos.repeat(reps, 1)[:ko].contiguous()
    bo = core.root_state[:, 1, :7].repeat(reps, 1)[:ko].contiguous()
    lines = []
    for run in range(2):
        for R in (16, 64, 1024):
            rays, parent = ray_set(R)
            dist, hits = torch.empty(k, R, device=dev), torch.empty(k, R, 8, device=dev)
            kw = dict(rays=rays, parent=parent, max_range=2.0)
            cases = [("raycast dist + hits", k, lambda: core.raycast(dist=dist, hits=hits, **kw), 36 * k * R),
                     ("raycast dist", k, lambda: core.raycast(dist=dist, **kw), 4 * k * R),
                     ("raycast hits", k, lambda: core.raycast(hits=hits, **kw), 32 * k * R)]
            if R == 16:
                do, ho = torch.empty(ko, R, device=dev), torch.empty(ko, R, 8, device=dev)
                cases.append(("raycast dist + hits, override", ko, lambda: core.raycast(dist=do, hits=ho, q=qo, box_pose=bo, **kw), 36 * ko * R))
            W, H = image_shape(R)
            cam = _abi.DexSimCamera()
            cam.width, cam.height, cam.hfov_deg, cam.near_clip, cam.far_clip, cam.parent_joint = W, H, 60.0, 0.01, 10.0, -1
            cam.eye[:], cam.target[:] = (-0.4, 0.0, 0.5), (0.0, 0.0, 0.2)
            scene = torch.zeros(k, core.render_layout()[1], device=dev)
            depth = torch.empty(k, H, W, device=dev)
            cases.append((f"render depth {W}x{H} (yardstick)", k, lambda: core.render(cam, scene, depth=depth), 4 * k * R + 4 * scene.numel()))
            block = []
            for name, rows, fn, nbytes in cases:
                us = qt.measure(fn, args.launches, 20)
                block.append({"case": name, "rays": R, "rows": rows, "run": run, "launches": args.launches, "us": round(us, 1),
                              "ns_per_ray": round(1000.0 * us / (rows * R), 3), "bytes_written": nbytes,
                              "write_floor_us": round(nbytes / HBM_BYTES_PER_US, 2)})
            yard = block[-1]["us"]
            for x in block:
                x["vs_render"] = round(x["us"] * k / (x["rows"] * yard), 3)       # per row, against one image per env
                qt.emit(x)
            lines += block
    qt.write(args, lines, [("case", "case"), ("rays", "rays"), ("rows", "rows"), ("run", "run"), ("us / call", "us"), ("ns / ray", "ns_per_ray"),
                           ("write floor us", "write_floor_us"), ("x render", "vs_render")])
    env.close()


if __name__ == "__main__":
    main()
