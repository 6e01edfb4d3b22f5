#!/usr/bin/env python3
"""Register / scratch / LDS use of every kernel in the BUILT librtx_hip.so (seconds; no recompile): the gfx950 code object is cut out of the
.hip_fatbin bundle and its metadata notes are read with llvm-readelf. Usage: scripts/kernel_budget.py [pattern]
  --insts          also disassemble (llvm-objdump) and count each kernel's instructions: all, VALU, v_readlane / v_writelane, s_load
  --against LIB    a second library (e.g. a build with EXTRA=-DRT_SHADE_KARGS=0, or the parent commit's): one row per kernel, LIB's figures then this build's"""
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rustracer_amd", "csrc", "_build", "librtx_hip.so")
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def code_objects(lib=LIB):
    """the gfx950 code objects of the library's bundles, one per translation unit"""
    b = open(lib, "rb").read()
    codes, i = [], b.find(b"__CLANG_OFFLOAD_BUNDLE__")
    while i >= 0:  # one bundle per translation unit (rtx_hip.hip, rtx_shade.hip, ...)
        n = struct.unpack_from("<Q", b, i + 24)[0]
        p = i + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", b, p)
            p += 24
            triple = b[p:p + tl]
            p += tl
            if b"gfx950" in triple:
                codes.append(b[i + off:i + off + size])
        i = b.find(b"__CLANG_OFFLOAD_BUNDLE__", i + 24)
    if not codes:
        raise RuntimeError("no gfx950 code object in " + lib)
    return codes


def _demangled(names):
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.splitlines()
    return [d.split("(")[0].replace("void ", "") for d in dem]


def kernel_resources(lib=LIB):
    """{demangled kernel name: dict(vgpr, agpr, sgpr, scratch, lds, vgpr_spills, sgpr_spills, arg_offsets)}; arg_offsets: the kernarg offsets of the kernel's
    explicit arguments, in order"""
    notes = ""
    for code in code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(code)
            f.flush()
            notes += subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True, check=True).stdout
    out = {}
    for blk in re.split(r"\n  - \.agpr_count:", notes)[1:]:
        g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        args = re.split(r"\n      - ", blk.split(".args:")[1].split("\n    .group_segment_fixed_size")[0])[1:] if ".args:" in blk else []
        offsets = [int(re.search(r"\.offset:\s+(\d+)", a).group(1)) for a in args if not re.search(r"\.value_kind:\s+hidden_", a)]
        out[name] = dict(vgpr=g("vgpr_count"), agpr=int(blk.split()[0]), sgpr=g("sgpr_count"), scratch=g("private_segment_fixed_size"),
                         lds=g("group_segment_fixed_size"), vgpr_spills=g("vgpr_spill_count"), sgpr_spills=g("sgpr_spill_count"), arg_offsets=offsets)
    names = list(out)
    return {d: out[n] for d, n in zip(_demangled(names), names)}


def kernel_instructions(lib=LIB, pattern=""):
    """{demangled kernel name: dict(insts, valu, readlane, writelane, s_load)} from the disassembly of the kernels whose mangled name holds `pattern`'s first word"""
    out = {}
    for code in code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(code)
            f.flush()
            text = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", f.name], capture_output=True, text=True, check=True).stdout
        for blk in re.split(r"\n(?=[0-9a-f]+ <)", text):
            m = re.match(r"[0-9a-f]+ <([^>]+)>:", blk)
            if not m or pattern not in m.group(1):
                continue
            ops = [l.split()[0] for l in blk.splitlines()[1:] if l.startswith("\t") and l.split()]
            out[m.group(1)] = dict(insts=len(ops), valu=sum(o.startswith("v_") for o in ops), readlane=sum(o.startswith("v_readlane") for o in ops),
                                   writelane=sum(o.startswith("v_writelane") for o in ops), s_load=sum(o.startswith("s_load") for o in ops))
    names = list(out)
    return {d: out[n] for d, n in zip(_demangled(names), names)}


def _row(v, ins):
    s = f"vgpr={v['vgpr']:4d} spills={v['vgpr_spills']:3d} scratch={v['scratch']:5d} sgpr_spills={v['sgpr_spills']:4d} lds={v['lds']:6d}"
    if ins is not None:
        s += f" insts={ins['insts']:6d} valu={ins['valu']:6d} readlane={ins['readlane']:4d} writelane={ins['writelane']:4d} s_load={ins['s_load']:4d}"
    return s


if __name__ == "__main__":
    argv = sys.argv[1:]
    insts = "--insts" in argv
    other = argv[argv.index("--against") + 1] if "--against" in argv else None
    rest = [a for k, a in enumerate(argv) if a not in ("--insts", "--against") and (k == 0 or argv[k - 1] != "--against")]
    pat = rest[0] if rest else ""
    mangled_pat = re.split(r"[<:, ]", pat.replace("rtx::", ""))[0]
    libs = ([other] if other else []) + [LIB]
    res = [kernel_resources(l) for l in libs]
    ins = [kernel_instructions(l, mangled_pat) if insts else {} for l in libs]
    for k in sorted(res[-1]):
        if pat in k:
            for j, l in enumerate(libs):
                if k in res[j]:
                    print(f"{k[:64]:64s} {'A' if other and j == 0 else ('B' if other else ' ')} {_row(res[j][k], ins[j].get(k) if insts else None)}")
