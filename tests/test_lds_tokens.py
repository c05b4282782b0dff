"""The LDS tokens of the step kernels (csrc/dexsim_device.h: lds_tok_load / lds_tok_store / lds_cnt_load) must compile to DS
instructions.  A volatile access through a generic pointer is not rewritten by the compiler's address-space inference: it becomes
a FLAT load or store (waited for with vmcnt(0) lgkmcnt(0), not ordered with the DS instructions next to it), which is what the
token waits were before they got a facility of their own.  Static checks on the device code of the step unit, built with the
product's CODEGEN_FLAGS: no instance of k_physics4 / k_physics1 holds an instruction whose mnemonic starts with `flat_`, and every
instance still uses 0 bytes of scratch.

The device code comes from the built library (the .hip_fatbin section's gfx950 code object, disassembled with the LLVM tools that
ship with hipcc); where those tools are missing, from one `-S --cuda-device-only` compile of the step unit per session."""
import functools
import os
import re
import shutil
import struct
import subprocess
import tempfile


from dexrobot_isaac_amd import build as B

KERNEL = re.compile(r"^_Z10k_physics[14]ILb[01]ELb[01]EE")      # k_physics4<GATED, MS>, k_physics1<GATED, MS>
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _llvm_bin():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    roots = [os.environ.get("ROCM_PATH"), os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "/opt/rocm"]
    for root in roots:
        d = root and os.path.join(root, "lib", "llvm", "bin")
        if d and all(os.path.exists(os.path.join(d, t)) for t in ("llvm-objcopy", "llvm-objdump", "llvm-readelf")):
            return d
    return None


def _code_objects(fatbin):
    """The gfx950 code objects of a .hip_fatbin section: one uncompressed offload bundle per translation unit."""
    out = []
    for m in re.finditer(re.escape(BUNDLE_MAGIC), fatbin):
        base = m.start()
        (n,) = struct.unpack_from("<Q", fatbin, base + len(BUNDLE_MAGIC))
        p = base + len(BUNDLE_MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", fatbin, p)
            triple = fatbin[p + 24: p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple and size:
                out.append(fatbin[base + off: base + off + size])
    return out


def _from_library(llvm, tmp):
    fat = os.path.join(tmp, "fat.bin")
    subprocess.check_call([os.path.join(llvm, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", B.LIB, os.path.join(tmp, "lib.copy")])
    kernels = {}
    with open(fat, "rb") as f:
        objects = _code_objects(f.read())
    for i, co in enumerate(objects):
        path = os.path.join(tmp, f"unit{i}.co")
        with open(path, "wb") as f:
            f.write(co)
        dis = subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", "--no-show-raw-insn", path], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
            if m:
                cur = kernels.setdefault(m.group(1), {"mnemonics": []}) if KERNEL.match(m.group(1)) else None
            elif cur is not None and line.startswith("\t") and line.split():
                cur["mnemonics"].append(line.split()[0])
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", path], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in notes.splitlines():      # (a kernel's keys are sorted: .name, then .private_segment_fixed_size, ..., .vgpr_count)
            m = re.match(r"^\s*-?\s*\.(name|private_segment_fixed_size|vgpr_count):\s+(\S+)", line)
            if not m:
                continue
            if m.group(1) == "name":
                cur = kernels.get(m.group(2)) if KERNEL.match(m.group(2)) else None
            elif cur is not None:
                cur["scratch" if m.group(1) == "private_segment_fixed_size" else "vgpr"] = int(m.group(2))
    return kernels


def _from_compile(tmp):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    asm = os.path.join(tmp, "step.s")
    subprocess.check_call([hipcc, *B.CODEGEN_FLAGS, "--cuda-device-only", "-S", "-o", asm, os.path.join(B.CSRC, B.SOURCES["step"][0])], cwd=B.CSRC)
    with open(asm) as f:
        txt = f.read()
    kernels = {}
    for m in re.finditer(r"^(_Z10k_physics[14]ILb[01]ELb[01]EE\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M):
        name, body = m.group(1), m.group(2)
        word = lambda key: int(re.search(rf"\.set {re.escape(name)}\.{key}, (\d+)", txt).group(1))
        kernels[name] = {"mnemonics": [ln.split()[0] for ln in body.splitlines() if ln.startswith("\t") and not ln.strip().startswith((".", ";"))],
                         "scratch": word("private_seg_size"), "vgpr": word("num_vgpr")}
    return kernels


@functools.lru_cache(maxsize=None)
def step_kernels():
    """{mangled name: {"mnemonics": [...], "scratch": bytes, "vgpr": count}} of the eight instances, once per session."""
    llvm = _llvm_bin()
    with tempfile.TemporaryDirectory() as tmp:
        if llvm is not None and os.path.exists(B.LIB):
            return _from_library(llvm, tmp)
        return _from_compile(tmp)


def test_the_eight_instances_are_found_and_really_parsed():
    k = step_kernels()
    assert len(k) == 8, sorted(k)
    for name, rec in k.items():
        assert len(rec["mnemonics"]) > 10000 and "ds_read_b32" in rec["mnemonics"] and "s_barrier" in rec["mnemonics"], name
        assert "scratch" in rec and "vgpr" in rec, name
        print(f"{name[:26]}  {len(rec['mnemonics'])} instructions, {rec['vgpr']} VGPRs, {rec['scratch']} B scratch")


def test_no_flat_instruction_in_the_step_kernels():
    for name, rec in step_kernels().items():
        flat = [m for m in rec["mnemonics"] if m.startswith("flat_")]
        assert not flat, f"{name}: {len(flat)} FLAT instructions ({sorted(set(flat))}): a token access is not typed as LDS"


def test_the_step_kernels_use_no_scratch():
    for name, rec in step_kernels().items():
        assert rec["scratch"] == 0, f"{name}: {rec['scratch']} bytes of scratch"
