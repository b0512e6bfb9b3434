"""Scalar-register spills of k_encode_local for 16-bit samples in blocks of 16, read off the built library: the kernel is
bound by vector-instruction issue, and a scalar register that does not fit is kept in a lane of a vector register -- every
save and reload is a vector instruction of its own (profiles/r21/README.md).  The figure is `.sgpr_spill_count` of the
kernel's entry in the code object's metadata note; no assembly is read.

The library holds one offload bundle per translation unit in its .hip_fatbin section (the clang-offload-bundler layout:
magic, entry count, then per entry offset, size, length of the target name, target name); the gfx950 code objects are cut
out with llvm-objcopy and their notes printed by llvm-readelf, both from the ROCm tree."""
import os
import re
import shutil
import struct
import subprocess

import pytest

from helpers import ROOT

LIB = os.path.join(ROOT, "libaec_amd", "lib", "libaec.so.0")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
# what the kernels were brought to (the parent: 39 and 48)
REACHED = {"k_encode_localILi16ELi2ELb1E": 0, "k_encode_localILi16ELi2ELb0E": 0}


def llvm_tool(name):
    for d in (os.environ.get("ROCM_PATH", "/opt/rocm"), "/opt/rocm"):
        p = os.path.join(d, "llvm", "bin", name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


def gfx950_code_objects(fatbin):
    at = fatbin.find(MAGIC)
    while at >= 0:
        (count,) = struct.unpack_from("<Q", fatbin, at + len(MAGIC))
        pos = at + len(MAGIC) + 8
        for _ in range(count):
            offset, size, tlen = struct.unpack_from("<QQQ", fatbin, pos)
            target = fatbin[pos + 24:pos + 24 + tlen].decode()
            pos += 24 + tlen
            if "gfx950" in target and size:
                yield fatbin[at + offset:at + offset + size]
        at = fatbin.find(MAGIC, at + len(MAGIC))


def spill_counts(tmp_path):
    """{kernel symbol: .sgpr_spill_count} over every gfx950 code object of the library"""
    objcopy, readelf = llvm_tool("llvm-objcopy"), llvm_tool("llvm-readelf")
    if not objcopy or not readelf:
        pytest.skip("no llvm-objcopy / llvm-readelf")
    fat = str(tmp_path / "fat.bin")
    subprocess.run([objcopy, "--dump-section", ".hip_fatbin=" + fat, LIB, str(tmp_path / "rest.so")], check=True)
    out = {}
    for i, co in enumerate(gfx950_code_objects(open(fat, "rb").read())):
        path = str(tmp_path / f"co{i}.elf")
        open(path, "wb").write(co)
        notes = subprocess.run([readelf, "--notes", path], check=True, capture_output=True, text=True).stdout
        spills = None
        # (a kernel's keys come in alphabetical order: .sgpr_spill_count, then .symbol)
        for key, value in re.findall(r"^\s+(\.sgpr_spill_count|\.symbol):\s+(\S+)", notes, flags=re.M):
            if key == ".sgpr_spill_count":
                spills = int(value)
            else:
                out[value.strip("'\"")] = spills
                spills = None
    return out


def test_local_encode_keeps_its_scalar_registers(tmp_path):
    assert os.path.exists(LIB), "build() has not run"
    counts = spill_counts(tmp_path)
    assert len(counts) > 100, "the code objects' notes were not read"
    for name, reached in REACHED.items():
        found = {s: n for s, n in counts.items() if name in s}
        assert len(found) == 1 and None not in found.values(), (name, found)
        (n,) = found.values()
        print(name, ".sgpr_spill_count", n)
        assert n <= reached, (name, n, "scalar spills are back: profiles/r21/README.md says where they came from")
