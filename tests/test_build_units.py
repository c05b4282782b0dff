"""The library's two translation units (build.SOURCES) without a compiler: the table covers csrc/ and says what the sources really
include, no kernel file belongs to both units, and build_lib recompiles exactly the units whose files changed."""
import os
import re

from dexrobot_isaac_amd import build


def _unit_files():
    return {name: {src, *deps} for name, (src, deps) in build.SOURCES.items()}


def test_unit_table_covers_csrc_and_shares_no_kernel_file():
    units = _unit_files()
    assert [src for src, _ in build.SOURCES.values()] == ["dexsim.hip", "dexsim_queries.hip"]      # link order: the step unit first
    assert set().union(*units.values()) == set(os.listdir(build.CSRC))
    assert {f for f in units["step"] & units["queries"]} == {"dexsim_device.h", "dexsim_host.h"}   # in particular no .hip.inc
    for name, files in units.items():   # the table is what the files include: nothing of csrc/ reaches a unit unlisted
        for f in files:
            text = open(os.path.join(build.CSRC, f)).read()
            local = {inc for inc in re.findall(r'^\s*#include "([^"/]+)"', text, re.M)}
            assert local <= files, (name, f, local - files)


def test_rebuild_compiles_only_the_units_whose_files_changed(monkeypatch, tmp_path):
    csrc, abi, lib = tmp_path / "csrc", tmp_path / "dexsim.h", str(tmp_path / "out" / "libdexsim.so")
    csrc.mkdir()
    (tmp_path / "out").mkdir()
    clock = [1000.0]

    def touch(path):   # every write gets a later time of its own: no reliance on the file system's resolution
        clock[0] += 10.0
        open(path, "a").close()
        os.utime(path, (clock[0], clock[0]))

    for files in _unit_files().values():
        for f in files:
            touch(csrc / f)
    touch(abi)
    monkeypatch.setattr(build, "CSRC", str(csrc))
    monkeypatch.setattr(build, "ABI_HEADER", str(abi))
    calls = []

    def fake_hipcc(cmd, **kw):
        calls.append(cmd)
        touch(cmd[cmd.index("-o") + 1])

    monkeypatch.setattr(build.subprocess, "check_call", fake_hipcc)

    def commands():   # ("compile", source) ... ("link",) of the build_lib call just made
        done = [("compile", os.path.basename(c[-1])) if "-c" in c else ("link",) for c in calls]
        calls.clear()
        return sorted(done[:-1]) + done[-1:] if done else []

    both = [("compile", "dexsim.hip"), ("compile", "dexsim_queries.hip"), ("link",)]
    assert build.build_lib(out=lib) == lib and commands() == both                       # nothing built yet
    assert build.build_lib(out=lib) == lib and commands() == []                         # nothing touched
    touch(csrc / "dexsim_invdyn.hip.inc")
    assert build.build_lib(out=lib) == lib and commands() == [("compile", "dexsim_queries.hip"), ("link",)]
    touch(csrc / "dexsim_physics.hip.inc")
    assert build.build_lib(out=lib) == lib and commands() == [("compile", "dexsim.hip"), ("link",)]
    touch(csrc / "dexsim_device.h")
    assert build.build_lib(out=lib) == lib and commands() == both
    touch(abi)
    assert build.build_lib(out=lib) == lib and commands() == both
    assert build.build_lib(out=lib) == lib and commands() == []
    os.remove(lib[:-len(".so")] + ".queries.o")                                         # a fresh library does not need its objects
    assert build.build_lib(out=lib) == lib and commands() == []
    touch(csrc / "dexsim_l2.hip.inc")                                                   # ... a stale one needs them all
    assert build.build_lib(out=lib) == lib and commands() == both
    assert build.build_lib(force=True, out=lib) == lib and commands() == both
