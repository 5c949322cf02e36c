#!/usr/bin/env python3
"""Device code of a source tree, kernel by kernel: compiles every translation unit of viterbidecodercpp_amd/csrc that holds kernels
for gfx950 (device side only, no GPU needed) and prints, per kernel symbol, the SHA-256 of its 64-byte descriptor (<name>.kd, without the
offset from the descriptor to the code) and of its code bytes.  With --jit the run-time compiled units of three geometries are added (a specialised K = 7 set, a K = 9 set, the
GENERIC K = 5 object: taken from the tree's package cache, compiled through vit_hip_precompile when missing; needs the built library).

    python scripts/compare_device_code.py [--jit] TREE > table.txt        # one tree
    python scripts/compare_device_code.py [--jit] TREE --against OTHER    # exit status 1 unless both trees hold the same kernels,
                                                                          # byte for byte, and TREE names none twice

A refactor of the host side must leave this table as it was.
"""
import argparse
import ctypes
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
JIT_SETS = [(7, 2, (91, 121)), (9, 2, (369, 491)), (5, 2, (0, 0))]


def run(cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def kernels_of_elf(path):
    """{kernel name: (sha256 of the descriptor, sha256 of the code, code bytes)} of a bare gfx950 ELF"""
    sections = {}           # index -> (address, file offset)
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S*\s+\S+\s+([0-9a-f]{16})\s+([0-9a-f]+)\s+([0-9a-f]+)", run([LLVM + "/llvm-readelf", "-SW", path]), re.M):
        sections[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
    syms = {}
    for line in run([LLVM + "/llvm-readelf", "-sW", path]).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6].isdigit():
            syms[f[7]] = (int(f[1], 16), int(f[2]), int(f[6]))
    blob = open(path, "rb").read()

    def body(name):
        value, size, shndx = syms[name]
        addr, off = sections[shndx]
        return blob[off + value - addr: off + value - addr + size]

    out = {}
    for name in syms:
        if name.endswith(".kd") and name[:-3] in syms:
            kd, code = body(name), body(name[:-3])
            assert len(kd) == 64, (name, len(kd))
            # bytes 16..23 are kernel_code_entry_byte_offset, the distance from the descriptor to the code: a property of the
            # unit's layout (it moves when another kernel joins or leaves the unit), not of the kernel -- left out of the hash
            kd = kd[:16] + kd[24:]
            out[name[:-3]] = (hashlib.sha256(kd).hexdigest()[:16], hashlib.sha256(code).hexdigest()[:16], len(code))
    return out


def units_of(tree):
    csrc = os.path.join(tree, "viterbidecodercpp_amd", "csrc")
    ids = re.search(r"^REG_IDS\s*:=\s*(.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).split()
    units = []
    for src in sorted(glob.glob(os.path.join(csrc, "*.hip"))):
        if os.path.basename(src) == "reg_inst.hip":
            units += [(src, ["-DVIT_REG_ID=" + i], "reg_inst_" + i) for i in ids]
        else:
            units.append((src, [], os.path.basename(src)[:-4]))
    return units


def compile_unit(unit, tmp):
    src, defs, label = unit
    obj = os.path.join(tmp, label + ".elf")
    run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "--no-gpu-bundle-output", "-c", *defs, "-o", obj, src])
    return label, kernels_of_elf(obj)


def jit_units(tree, tmp):
    lib = ctypes.CDLL(os.path.join(tree, "viterbidecodercpp_amd", "libvit_hip.so"))
    lib.vit_hip_last_error.restype = ctypes.c_char_p
    out = []
    for K, R, G in JIT_SETS:
        path = ctypes.create_string_buffer(4096)
        poly = (ctypes.c_uint32 * 6)(*G)
        if lib.vit_hip_precompile(K, R, poly, 2, None, path, ctypes.c_size_t(4096)) != 0:
            raise RuntimeError(lib.vit_hip_last_error().decode())
        label = "jit_K%dR%d_%s" % (K, R, "_".join(map(str, G)))
        elf = os.path.join(tmp, label + ".elf")
        run([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
             "--input=" + path.value.decode(), "--output=" + elf])
        out.append((label, kernels_of_elf(elf)))
    return out


def table_of(tree, jit):
    """[(unit, kernel, kd hash, code hash, code bytes)], and the names that more than one ahead-of-time unit holds"""
    with tempfile.TemporaryDirectory() as tmp:
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            per_unit = list(pool.map(lambda u: compile_unit(u, tmp), units_of(tree)))
        seen, twice = set(), []
        for _, kernels in per_unit:
            twice += [k for k in kernels if k in seen]
            seen |= set(kernels)
        if jit:
            per_unit += jit_units(tree, tmp)
    rows = [(unit, k) + v for unit, kernels in per_unit for k, v in sorted(kernels.items())]
    return rows, twice


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree")
    ap.add_argument("--against", help="another tree: fail unless the kernels are the same, byte for byte")
    ap.add_argument("--jit", action="store_true", help="add the run-time compiled units (needs each tree's built library)")
    a = ap.parse_args()
    rows, twice = table_of(a.tree, a.jit)
    print("# unit  kernel  sha256(descriptor)[:16]  sha256(code)[:16]  code bytes")
    for r in rows:
        print("%s  %s  %s  %s  %d" % r)
    print("# %d kernels in %d units; names held twice: %s" % (len(rows), len({r[0] for r in rows}), ", ".join(twice) or "none"))
    bad = bool(twice)
    if a.against:
        # a kernel keeps its name, not its unit (jit units keep theirs: the same kernel names recur in each)
        key = lambda r: (r[0] if r[0].startswith("jit_") else "", r[1])
        mine = {key(r): r[2:] for r in rows}
        theirs = {key(r): r[2:] for r in table_of(a.against, a.jit)[0]}
        for k in sorted(set(mine) | set(theirs)):
            if mine.get(k) != theirs.get(k):
                bad = True
                print("# DIFFERENT %s%s: %s here, %s in %s" % (k[0] and k[0] + " ", k[1], mine.get(k, "absent"), theirs.get(k, "absent"), a.against))
        print("# against %s: %s" % (a.against, "DIFFERENT" if bad else "%d kernels identical (descriptor and code bytes)" % len(mine)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
