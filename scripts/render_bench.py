"""Cost of the camera sensors (dexsim_render) on the GPU.

Shapes: N = 4096 envs at 64 x 64 with all three outputs and with depth only; one env at 1280 x 720.  Every shape is warmed up,
then at least `--launches` renders (and at least `--min-seconds` of them) are enqueued back to back inside ONE timed region
that ends in a device synchronise (a render is two launches: scene records + rays).  Reported per shape: microseconds per render, rays per second, and the two bounds that frame
them, computed from the shapes:
  * bytes: the output images (4 B depth + 4 B seg + 4 B rgba per pixel) over the measured HBM copy rate (6.29 TB/s);
  * flops: rays x FLOP_PER_RAY over the FP32 vector peak (157.3 TFLOP/s, which counts an FMA as two) -- FLOP_PER_RAY counts the
    arithmetic of the ray kernel's source: ray set-up, ground, box slabs, 18 capsules (3 dots, cylinder quadratic, two spheres,
    the diffuse term), selection and shading;
  * VALU issue: rays x VALU_PER_RAY over the chip's vector issue rate (1 024 SIMDs x 64 lanes every 2 cycles at 2.4 GHz =
    7.86e13 lane-instructions/s, i.e. the same peak counted in instructions instead of FMAs) -- VALU_PER_RAY is the number of
    vector instructions in the ray kernel's ISA (k_render_rays<true>, counted in the compiler's output of this source).
Prints one JSON line.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.29e12
FP32_FLOP_PER_S = 157.3e12
# ray set-up 40 | ground 4 | box 60 | per capsule: 3 dot products 15, body 14, two spheres 14, n.l 5, selects 10 | shading 20
VALU_LANE_INSTR_PER_S = 1024 * 64 / 2 * 2.4e9
VALU_PER_RAY = 1601
FLOP_PER_RAY = 40 + 4 + 60 + 18 * (15 + 14 + 14 + 5 + 10) + 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--num-envs", type=int, default=4096)
    args = ap.parse_args()
    import torch
    from dexrobot_isaac_amd import _abi
    from dexrobot_isaac_amd.config import build_sim_config, default_cfg
    from dexrobot_isaac_amd.core import DexSimCore
    if not torch.cuda.is_available():
        raise SystemExit("render_bench needs a GPU")
    cfg = default_cfg("BlindGrasping")
    cfg["env"]["numEnvs"] = args.num_envs
    sc, model = build_sim_config(cfg)
    core = DexSimCore(sc, model.to_struct(), "cuda:0")
    core.reset()
    g = torch.Generator().manual_seed(0)
    for _ in range(20):                                           # spread the poses
        core.step((2 * torch.rand(args.num_envs, 18, generator=g) - 1).cuda())
    words = core.render_layout()[1]

    def camera(w, h):
        cam = _abi.DexSimCamera()
        cam.width, cam.height, cam.hfov_deg, cam.near_clip, cam.far_clip, cam.parent_joint = w, h, 75.0, 0.01, 10.0, -1
        for i, (e, t) in enumerate(zip((-0.45, 0.3, 0.65), (0.0, 0.0, 0.3))):
            cam.eye[i], cam.target[i] = e, t
        return cam

    results = []
    for name, w, h, ids, outs in (("n4096_64x64_all", 64, 64, None, ("depth", "rgba", "seg")),
                                  ("n4096_64x64_depth", 64, 64, None, ("depth",)),
                                  ("n1_1280x720_all", 1280, 720, [0], ("depth", "rgba", "seg"))):
        k = args.num_envs if ids is None else len(ids)
        cam = camera(w, h)
        scene = torch.zeros(k, words, device="cuda:0")
        bufs = {"depth": torch.zeros(k, h, w, device="cuda:0"), "rgba": torch.zeros(k, h, w, 4, dtype=torch.uint8, device="cuda:0"),
                "seg": torch.zeros(k, h, w, dtype=torch.int32, device="cuda:0")}
        kw = {o: bufs[o] for o in outs}
        idt = None if ids is None else torch.tensor(ids, device="cuda:0")
        for _ in range(args.warmup):
            core.render(cam, scene, env_ids=idt, **kw)
        def timed(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                core.render(cam, scene, env_ids=idt, **kw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n
        n = max(args.launches, int(args.min_seconds / timed(20)) + 1)     # a timed region of at least --min-seconds
        us = timed(n) * 1e6
        rays = k * w * h
        hit = float((bufs[outs[0]] != (float("inf") if outs[0] == "depth" else 0)).float().mean()) if outs[0] != "rgba" else None
        t_bytes = rays * 4 * len(outs) / HBM_BYTES_PER_S * 1e6
        t_flops = rays * FLOP_PER_RAY / FP32_FLOP_PER_S * 1e6
        t_valu = rays * VALU_PER_RAY / VALU_LANE_INSTR_PER_S * 1e6
        results.append({"shape": name, "us_per_render": round(us, 2), "rays_per_s": round(rays / us * 1e6, 0), "rays": rays, "launches": n,
                        "bound_bytes_us": round(t_bytes, 2), "bound_flops_us": round(t_flops, 2),
                        "bound_valu_issue_us": round(t_valu, 2), "binding_bound": "flops" if t_flops > t_bytes else "bytes",
                        "share_of_bound": round(max(t_bytes, t_flops) / us, 3), "hit_share": hit})
    print(json.dumps({"metric": "render", "launches": args.launches, "flop_per_ray": FLOP_PER_RAY, "results": results}))


if __name__ == "__main__":
    main()
