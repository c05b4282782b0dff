"""Build libdexsim.so (HIP, gfx950 only) in-tree with hipcc.  No JIT cache: the .so sits next to the package
so that it travels with the repo snapshot and shows up as loaded native code."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libdexsim.so")
ABI_HEADER = os.path.join(HERE, "..", "include", "dexsim.h")
ABI_PARTS = ["dexsim_fk.h", "dexsim_ray.h"]   # the files next to ABI_HEADER that it includes
_SHARED = ["dexsim_device.h", "dexsim_host.h"]
# The library's two translation units, in link order: name -> (source, the files of csrc/ that its compile reads besides).  Neither
# includes a .hip.inc of the other: the step kernels' code cannot depend on a query file, and a query edit does not recompile them.
SOURCES = {
    "step": ("dexsim.hip", [*_SHARED, "dexsim_stamps.h", "dexsim_physics.hip.inc", "dexsim_l2.hip.inc", "dexsim_state.hip.inc"]),
    "queries": ("dexsim_queries.hip", [*_SHARED, "dexsim_chain.hip.inc", "dexsim_render.hip.inc", "dexsim_kindyn.hip.inc",
                                       "dexsim_ik.hip.inc", "dexsim_proximity.hip.inc", "dexsim_raycast.hip.inc",
                                       "dexsim_invdyn.hip.inc", "dexsim_fk.hip.inc", "dexsim_fwddyn.hip.inc",
                                       "dexsim_dynderiv.hip.inc"]),
}


DEBUG_SPIN_LIB = os.path.join(HERE, "libdexsim_dbgspin.so")
# the code-generation flags of the library (reasons: build_lib); tests that compile device code of the library stand-alone use the same
CODEGEN_FLAGS = ["--offload-arch=gfx950", "-O3", "-fno-slp-vectorize", "-fno-hip-fp32-correctly-rounded-divide-sqrt",
                 "-mllvm", "-amdgpu-sched-strategy=max-ilp", "-std=c++17"]


def build_debug_spin(force=False, bound=2000000):
    """Diagnostic twin of the library with every LDS token wait bounded (-DDEXSIM_DEBUG_SPIN=<polls>, see
    dexsim_physics.hip.inc): a sequencing bug shows up as a recorded word in the counters block instead of a hung GPU.
    Loaded only by tests/ (DEXSIM_LIB_PATH); the product never uses it."""
    return build_lib(force=force, defs=(f"-DDEXSIM_DEBUG_SPIN={int(bound)}",), out=DEBUG_SPIN_LIB)


PROFILE_LIB = os.path.join(HERE, "..", "build_variants", "libdexsim_prof.so")


def build_profile(detail=None, extra_defs=(), out=PROFILE_LIB, force=True):
    """Profiling twin of the library (-DDEXSIM_PROFILE_PHASES: per-wave cycle stamps, csrc/dexsim_stamps.h), for
    scripts/phase_profile.py.  detail: the detail groups of the header's list to compile in, a name or several ("SCHUR",
    ("SCHUR", "SWEEP05"), "NONE"); None = the header's default.  extra_defs: further -D experiment switches.  Same code-generation
    flags as the product, so that the stamps time the kernel that ships; never built next to the package."""
    defs = ["-DDEXSIM_PROFILE_PHASES"]
    if detail:
        defs.append("-DDEXSIM_PROFILE_DETAIL=" + "|".join([detail] if isinstance(detail, str) else detail))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    return build_lib(force=force, defs=(*defs, *extra_defs), out=out)


def build_lib(force=False, verbose=False, defs=(), out=None):
    """hipcc --offload-arch=gfx950 (cross-compiles without a GPU): each unit of SOURCES to an object next to the library
    (libdexsim.step.o, libdexsim.queries.o), both at once, then one link.  Without `force` a unit is compiled only if its object is
    missing or older than one of its files, and a library newer than every file of both units is left alone whether or not the
    objects are still there.  Objects do not remember their defines: every caller that passes `defs` passes `force`.  Returns
    the path of the library."""
    lib = out or LIB
    units = []   # (source, object, newest modification time of what the compile reads)
    for name, (src, deps) in SOURCES.items():
        files = [os.path.join(CSRC, f) for f in (src, *deps)] + [ABI_HEADER, *(os.path.join(os.path.dirname(ABI_HEADER), f) for f in ABI_PARTS)]
        newest = max(os.path.getmtime(f) for f in files if os.path.exists(f))
        units.append((os.path.join(CSRC, src), f"{os.path.splitext(lib)[0]}.{name}.o", newest))
    if not force and os.path.exists(lib) and all(t <= os.path.getmtime(lib) for _, _, t in units):
        return lib
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found: libdexsim.so cannot be built on this machine")
    # -fno-slp-vectorize: the auto-vectoriser's v_pk_* pairs cost more v_mov shuffles and wait states than they
    # save here (13.8k -> 13.4k instructions, scratch 112 -> 48 B in k_substep); packed FP32 is written by hand
    # (f2) where it pays.
    # -fno-hip-fp32-correctly-rounded-divide-sqrt: fp32 `/` and sqrtf as the <= 2.5 ulp sequences (v_rcp / v_rsq + one
    # Newton step) instead of the correctly rounded ones (v_div_scale / v_div_fmas / v_div_fixup, ~10 instructions each): the
    # step kernel has ~60 divisions per wave and sub-step and is VALU-issue bound on the SIMDs that carry two finger waves
    # (75.4 -> 69.9 us per control step).  Still fp32 arithmetic; every parity test (golden vectors of the reference at 2e-5 /
    # 2e-6, oracle at the fp64-derived tolerance) holds unchanged -- 2.5 ulp is 3e-7 relative.
    # -mllvm -amdgpu-sched-strategy=max-ilp: the step kernel is a few long dependency chains on waves that are (almost) alone on
    # their SIMD, so the scheduler should interleave independent chains rather than minimise register pressure: same VGPR
    # counts, still no spills / scratch, 61.3 -> 62.2 M env-steps/s (contact-rich regime 187 -> 189 us: within 1 %).
    def run(cmd):
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd, cwd=CSRC)

    compiles = [[hipcc, *CODEGEN_FLAGS, "-fPIC", *defs, "-c", "-o", obj, src]
                for src, obj, t in units if force or not os.path.exists(obj) or os.path.getmtime(obj) < t]
    with ThreadPoolExecutor(len(SOURCES)) as pool:
        list(pool.map(run, compiles))
    # the library is missing or older than a file of a unit, hence older than that unit's object: always link
    run([hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", "-o", lib, *(obj for _, obj, _ in units)])
    return lib


if __name__ == "__main__":   # python -m dexrobot_isaac_amd.build [--out PATH] [-D...]: the library, or a variant of it with defines
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args, defs = ap.parse_known_args()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    print(build_lib(force=True, verbose=True, defs=tuple(defs), out=args.out))
