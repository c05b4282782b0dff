"""The profiling build's cycle stamps (csrc/dexsim_stamps.h) without a GPU: the row map as the C preprocessor expands it against the
one scripts/phase_profile.py reads, every stamped row inside `crow` and no row shared by two groups, and build_profile's command
line (the product's code-generation flags plus its defines, nothing else)."""
import importlib.util
import itertools
import os
import re
import shutil
import subprocess

import pytest

from dexrobot_isaac_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("first", "per_wave", "slots", "waves", "bodies", "detail")


def _script():
    spec = importlib.util.spec_from_file_location("phase_profile", os.path.join(ROOT, "scripts", "phase_profile.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def header():
    """(groups, rows of one body, rows of crow) from the preprocessor's expansion of the header's list"""
    crow = re.search(r"X\(float, crow, ([^)]*)\)", open(os.path.join(build.CSRC, "dexsim_device.h")).read()).group(1)
    src = ('#include "include/dexsim.h"\n#include "dexrobot_isaac_amd/csrc/dexsim_stamps.h"\n'
           "#define X(name, first, per_wave, slots, waves, bodies, detail) GROUP name first per_wave slots waves bodies detail ;\n"
           f"DEXSIM_PROFILE_GROUPS(X)\nBODY_ROWS DEXSIM_PROFILE_BODY_ROWS ;\nCROW_ROWS {crow} ;\n")
    cc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = subprocess.run([cc, "-x", "c++", "-E", "-P", "-I", ROOT, "-"], input=src, capture_output=True, text=True, check=True).stdout
    tail = out[out.rindex("GROUP BODY"):]
    groups = {m.group(1): dict(zip(KEYS, (int(v, 0) for v in m.group(2).split())))
              for m in re.finditer(r"GROUP (\w+) ([^;]*);", tail)}
    return groups, int(re.search(r"BODY_ROWS (\d+)", tail).group(1)), eval(re.search(r"CROW_ROWS ([^;]*);", tail).group(1))


def _rows(g, body_rows):
    return {g["first"] + body_rows * b + g["per_wave"] * w + s
            for b in range(g["bodies"]) for w in range(8) if (g["waves"] >> w) & 1 for s in range(g["slots"])}


def test_rows_inside_crow_for_every_body(header):
    groups, body_rows, crow_rows = header
    assert [body_rows * b for b in range(5)] == [0, 64, 128, 192, 256]      # the stamp bases of the single body and of k_physics4's four
    assert {n for n, g in groups.items() if g["bodies"] == 5} == {"BODY", "SWEEP05", "SCHUR", "PH2", "SWEEP_ALL"}
    for name, g in groups.items():
        rows = _rows(g, body_rows)
        assert g["bodies"] in (1, 5) and 0 < g["slots"] <= g["per_wave"] and 8 * g["per_wave"] <= body_rows, name
        assert min(rows) >= 0 and max(rows) < crow_rows, (name, min(rows), max(rows), crow_rows)


def test_groups_are_disjoint(header):
    """every set of detail groups can be compiled in together (the define is a bit mask), so no two groups may share a row"""
    groups, body_rows, _ = header
    for (na, a), (nb, b) in itertools.combinations(groups.items(), 2):
        assert not _rows(a, body_rows) & _rows(b, body_rows), (na, nb)
    bits = [g["detail"] for g in groups.values() if g["detail"]]
    assert all(b & (b - 1) == 0 for b in bits) and len(set(bits)) == len(bits)


def test_script_reader_agrees_with_header(header):
    groups, body_rows, _ = header
    s_groups, s_body_rows, s_default = _script().stamp_groups()
    assert list(s_groups) == list(groups) and s_body_rows == body_rows
    for name, g in groups.items():
        assert s_groups[name] == g, name
    assert groups[s_default]["detail"] != 0


def test_build_profile_command_line(monkeypatch, tmp_path):
    calls = []
    monkeypatch.setattr(build.subprocess, "check_call", lambda cmd, **kw: calls.append((cmd, kw)))
    out = str(tmp_path / "variants" / "libdexsim_prof.so")
    assert build.build_profile(detail=("SCHUR", "SWEEP05"), extra_defs=("-DEXP_X=1",), out=out) == out
    assert build.build_profile(out=out) == out
    assert build.build_profile(detail="PH2", out=out) == out
    tails = [["-DDEXSIM_PROFILE_PHASES", "-DDEXSIM_PROFILE_DETAIL=SCHUR|SWEEP05", "-DEXP_X=1"], ["-DDEXSIM_PROFILE_PHASES"],
             ["-DDEXSIM_PROFILE_PHASES", "-DDEXSIM_PROFILE_DETAIL=PH2"]]
    objs = [f"{out[:-len('.so')]}.{name}.o" for name in build.SOURCES]
    srcs = [os.path.join(build.CSRC, src) for src, _ in build.SOURCES.values()]
    per_build = len(srcs) + 1   # one compile per unit (both at once: in either order), then the link
    assert len(calls) == 3 * per_build
    for i, defs in enumerate(tails):
        *compiles, link = [cmd for cmd, kw in calls[per_build * i:per_build * (i + 1)]]
        assert all(os.path.basename(cmd[0]) == "hipcc" for cmd in (*compiles, link))
        assert sorted(cmd[1:] for cmd in compiles) == sorted([*build.CODEGEN_FLAGS, "-fPIC", *defs, "-c", "-o", obj, src]
                                                             for obj, src in zip(objs, srcs))
        assert link[1:] == ["--offload-arch=gfx950", "-fPIC", "-shared", "-o", out, *objs]
    assert os.path.abspath(build.PROFILE_LIB).startswith(os.path.join(ROOT, "build_variants") + os.sep)   # default: never next to the package
