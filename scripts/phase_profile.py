#!/usr/bin/env python
"""Diagnostic: builds the profiling twin of libdexsim (build.build_profile) and prints where a sub-step's cycles go (per wave,
s_memtime at the phase boundaries).  The product library is never built with this flag.
  python scripts/phase_profile.py [N [z]] [--detail=SCHUR,SWEEP05] [-DEXP_...]   (z: contact-rich regime, 4096 -0.40; detail groups and
row map: csrc/dexsim_stamps.h; -D...: experiment switches)"""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dexrobot_isaac_amd.build import CSRC, build_profile  # noqa: E402


def stamp_groups(header=os.path.join(CSRC, "dexsim_stamps.h")):
    """The header's DEXSIM_PROFILE_GROUPS list (name -> its columns), the rows of one body and the default detail group."""
    text = open(header).read()
    keys = ("first", "per_wave", "slots", "waves", "bodies", "detail")
    groups = {m.group(1): dict(zip(keys, (int(v, 0) for v in m.group(2).split(","))))
              for m in re.finditer(r"^\s*X\((\w+),([^)]*)\)", text, re.M)}
    return groups, int(re.search(r"#define DEXSIM_PROFILE_BODY_ROWS (\d+)", text).group(1)), re.search(r"#define DEXSIM_PROFILE_DETAIL (\w+)", text).group(1)


def main(argv):
    import torch
    from dexrobot_isaac_amd import _abi, _lib
    groups, body_rows, default_detail = stamp_groups()
    pos = [a for a in argv if not a.startswith(("-D", "--detail="))]
    detail = [d for d in next((a[9:] for a in argv if a.startswith("--detail=")), default_detail).split(",") if d != "NONE"]
    assert all(groups[d]["detail"] for d in detail), detail
    _lib.LIB_PATH = build_profile(detail=detail or "NONE", extra_defs=[a for a in argv if a.startswith("-D")])
    from dexrobot_isaac_amd.config import build_sim_config, default_cfg
    from dexrobot_isaac_amd.core import DexSimCore
    n = int(pos[0]) if pos else 4096
    cfg = default_cfg("BlindGrasping")
    cfg["env"]["numEnvs"] = n
    sc, model = build_sim_config(cfg)
    core = DexSimCore(sc, model.to_struct(), "cuda:0")
    core.reset()
    a = 2 * torch.rand(n, 18, device="cuda:0") - 1
    if len(pos) <= 1:
        for _ in range(10):
            core.step(a)
    else:   # contact-rich regime: python scripts/phase_profile.py 4096 -0.40  (scripts/contact_regime.py's state)
        g = torch.Generator(device="cuda:0").manual_seed(3)
        for z, nsteps in ((0.0, 120), (float(pos[1]), 120)):     # the same sequence of states as scripts/contact_regime.py
            q = core.field("q").zero_()
            q[2] = z
            q[6:] = 0.3 * torch.rand(20, n, device="cuda:0", generator=g)
            core.field("qd").zero_()
            core.field("targets").copy_(q)
            for _ in range(nsteps):
                core.physics_step(False)
        print("contact regime: contacts/env mean %.2f max %d" % (core.field("ncontact").float().mean().item(), int(core.field("ncontact").max().item())))
    lanes = np.arange(0, n, 64)

    def run(stage):   # one launch; returns the reader of its stamps: [workgroup][slot] of one wave of a group (lane 0 of every block)
        core.step(a) if stage is None else core.run_stage(_abi.STAGE[stage])
        torch.cuda.synchronize()
        crow = core.field("crow").view(torch.int32).cpu().numpy()
        def rows(group, wave, body=0, slots=None):
            g = groups[group]
            r0 = g["first"] + body_rows * body + g["per_wave"] * wave
            return crow[r0:r0 + (slots or g["slots"])][:, lanes].T
        return rows

    rows = run("SUBSTEP")
    names = ["base chain", "phase1 fingers|palm", "phase2 schur|narrow", "phase3 rows", "phase4 sweeps", "phase5 integrate", "publish",
             "(general path) end of sweep 1 / wave 6: of its first box block"]
    print(f"N={n}: cycles since kernel start at each boundary, median over {len(lanes)} workgroups (s_memtime @100 MHz ticks x?)")
    for wv in range(7):
        st = rows("BODY", wv)
        print(f"wave {wv}: " + "  ".join(f"{nm}={int(v)}" for nm, v in zip(names, np.median(st, axis=0))))
        if wv == 0 and "SCHUR" in detail:   # inside wave 0's Schur phase
            print("  wave 0, Schur phase: start %d, composite sum %d, own rows %d, tokens seen %d, S / tau_B complete %d, solved %d" % tuple(int(v) for v in np.median(rows("SCHUR", 0), axis=0)))
        for w in (1, 5) if wv == 0 and "PH2" in detail else ():   # inside phase 2 of the general path: waves 1 and 5
            ss = np.median(rows("PH2", w), axis=0)
            print(f"  wave {w}, phase 2: narrowphase done at {int(ss[0])}, barrier passed {int(ss[1])}, appended {int(ss[2])}")
        for w in (0, 5) if wv == 0 and "SWEEP05" in detail else ():   # inside pass 2 of the general path's sweeps: waves 0 and 5
            ss = np.median(rows("SWEEP05", w), axis=0)
            print(f"  wave {w}, sweep 2: starts at {int(ss[0])}, item done +{int(ss[1]-ss[0])}, barrier passed +{int(ss[2]-ss[1])}, reduction done +{int(ss[3]-ss[2])}, second barrier passed +{int(ss[4]-ss[3])}")
        if wv == 0:   # the launch ends with its slowest workgroup
            print("wave 0, slowest workgroup: " + "  ".join(f"{nm}={int(v)}" for nm, v in zip(names, st[np.argmax(st[:, 6])])))
            print("wave 0, publish stamp over workgroups: min %d  median %d  p90 %d  max %d" % (st[:, 6].min(), np.median(st[:, 6]), np.percentile(st[:, 6], 90), st[:, 6].max()))
    if "SWEEP_ALL" in detail:   # pass 2 of the sweeps, every wave
        print("pass 2 of the sweeps, per wave (median workgroup): start | own work done | first barrier passed | reduction done | second barrier passed")
        for wv in range(7):
            ss = np.median(rows("SWEEP_ALL", wv), axis=0)
            print(f"  wave {wv}: start {int(ss[0])}  work +{int(ss[1]-ss[0])}  B1 at {int(ss[2])} (+{int(ss[2]-ss[1])})  reduce +{int(ss[3]-ss[2])}  B2 at {int(ss[4])} (+{int(ss[4]-ss[3])})")

    # k_post: per-wave stamps after phase A, phase B (wave-0 logic), the row flush and the obs_buf flush; then wave 0's logic split
    rows = run("POST")
    pn = ["phase A", "phase B", "row flush", "obs_buf flush"]
    for wv in range(8):
        print(f"k_post wave {wv}: " + "  ".join(f"{nm}={int(v)}" for nm, v in zip(pn, np.median(rows("POST", wv), axis=0))))
    print("k_post logic (wave 0, from phase B start): " + "  ".join(f"{nm}={int(v)}" for nm, v in zip(
        ["task obs+FSM", "termination", "reward terms", "reward table", "stats"], np.median(rows("POST_LOGIC", 0), axis=0))))

    # the production launch: four bodies back to back (stamps are relative to each body's own start)
    rows = run("PHYSICS")
    for b in range(4):
        for wv in (0, 4, 5, 6):
            st = rows("BODY", wv, b + 1, 7 if b == 3 else 6)
            print(f"k_physics4 body {b} wave {wv}: " + "  ".join(f"{nm}={int(v)}" for nm, v in zip(names, np.median(st, axis=0))))

    # what a stamp tick is worth: the same launch timed with events, next to the sum of the four bodies' stamps of the median workgroup
    tot = sum(int(np.median(rows("BODY", 0, b + 1, 7 if b == 3 else 6), axis=0)[-1]) for b in range(4))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); core.run_stage(_abi.STAGE["PHYSICS"]); e1.record(); torch.cuda.synchronize()
    one = e0.elapsed_time(e1) * 1e3
    e0.record()
    for _ in range(20):
        core.run_stage(_abi.STAGE["PHYSICS"])
    e1.record(); torch.cuda.synchronize()
    many = e0.elapsed_time(e1) * 1e3 / 20
    print(f"k_physics4 (profile build): {tot} stamp ticks over the four bodies (wave 0, median workgroup); one launch {one:.1f} us, 20 back to back {many:.1f} us each -> {tot / many / 1e3:.2f} ticks per ns")

    # the whole control step as the product runs it, one launch: the last body's stamps for every wave -- who reaches the barrier in
    # front of the post block last -- and the post block's own (relative to its start)
    rows = run(None)
    print("full step, last body (median workgroup): phase 5 done | publication (+ the box wave's post pre-tasks) done")
    for wv in range(7):
        print("  wave %d: %d | %d" % (wv, *np.median(rows("BODY", wv, 4, 7), axis=0)[5:7]))
    for wv in range(7):
        print(f"  post block wave {wv}: " + "  ".join(f"{nm}={int(v)}" for nm, v in zip(pn, np.median(rows("POST", wv), axis=0))))


if __name__ == "__main__":
    main(sys.argv[1:])
