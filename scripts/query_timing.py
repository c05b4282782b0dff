"""What the timing scripts of the device queries share (kindyn_timing, invdyn_timing, fwddyn_timing, dynderiv_timing, ik_timing,
proximity_timing, state_copy_timing): the measurement rule, the posed core, the common arguments and the writers.  A module, not a
program; a script keeps its docstring, its cases, its yardsticks and its columns.

The measurement rule: one call, a warm-up block, then HIP events around blocks of `block` back-to-back launches until `launches`
launches ran; the figure is the mean per launch in microseconds.  The block length is the script's: a figure is comparable with
the committed profiles/*/*.jsonl only at the block length those were taken with."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

DEV = "cuda:0"


def time_block(fn, n):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1000.0          # us


def measure(fn, launches, block):
    fn()
    time_block(fn, block)                        # warm-up
    blocks = max(1, (launches + block - 1) // block)
    return sum(time_block(fn, block) for _ in range(blocks)) / (blocks * block)


def blind_grasping_core(n):
    """A DexSimCore of n BlindGrasping envs, reset."""
    from dexrobot_isaac_amd.config import build_sim_config, default_cfg
    from dexrobot_isaac_amd.core import DexSimCore
    cfg = default_cfg("BlindGrasping")
    cfg["env"]["numEnvs"] = n
    sc, model = build_sim_config(cfg)
    core = DexSimCore(sc, model.to_struct(), DEV)
    core.reset()
    return core


class Draws:
    """The seeded device stream the set-ups draw from, in the order of the calls: poses inside the joint limits of `core`, and
    rates uniform in [-a, a]."""

    def __init__(self, core, seed=0):
        self.g = torch.Generator(device=DEV).manual_seed(seed)
        self.lo, self.hi = torch.tensor(list(core.model.lo), device=DEV), torch.tensor(list(core.model.hi), device=DEV)

    def pose(self, rows):
        return self.lo + (self.hi - self.lo) * torch.rand(rows, len(self.lo), device=DEV, generator=self.g)

    def sym(self, a, *shape):
        return a * (2 * torch.rand(*shape, device=DEV, generator=self.g) - 1)


def posed_core(n, speed=None):
    """(core, draws): blind_grasping_core(n) at a random pose inside the limits and, with `speed`, joint rates in [-speed, speed]."""
    core = blind_grasping_core(n)
    draws = Draws(core)
    core.dof_state[:, :, 0] = draws.pose(n)
    if speed is not None:
        core.dof_state[:, :, 1] = draws.sym(speed, n, core.dof_state.shape[1])
    core.set_dof_state_indexed(torch.arange(n, device=DEV))
    return core, draws


def add_ratio(block, key, yardstick, digits):
    """block[i][key] = us of the line / us of the line of the same row count whose case starts with `yardstick`."""
    for x in block:
        ref = next(y for y in block if y["case"].startswith(yardstick) and y["rows"] == x["rows"])
        x[key] = round(x["us"] / ref["us"], digits)


def parser(launches, num_envs=None, rows=None, override_rows=False, tag=False, readme=False):
    """The arguments the scripts share; a script adds its own to the parser returned."""
    ap = argparse.ArgumentParser()
    if num_envs is not None:
        ap.add_argument("--num-envs", type=int, nargs="+", default=num_envs)
    if rows is not None:
        ap.add_argument("--rows", type=int, default=rows)
    if override_rows:
        ap.add_argument("--override-rows", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=launches)
    if tag:
        ap.add_argument("--tag", default="", help="names the build in the JSON lines")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    if readme:
        ap.add_argument("--readme", default=None, help="write the table of this run (markdown) to this file")
    return ap


def emit(line):
    print(json.dumps(line), flush=True)


def table(lines, columns):
    """Markdown table of `lines`; columns: (header, key) pairs."""
    out = ["| " + " | ".join(h for h, _ in columns) + " |", "|---" * len(columns) + "|"]
    out += ["| " + " | ".join(str(x[k]) for _, k in columns) + " |" for x in lines]
    return "\n".join(out) + "\n"


def write(args, lines, columns=None):
    """Append the JSON lines to --out and, for a script with `columns`, write their table to --readme."""
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    if columns and args.readme:
        os.makedirs(os.path.dirname(os.path.abspath(args.readme)), exist_ok=True)
        with open(args.readme, "w") as f:
            f.write(table(lines, columns))
