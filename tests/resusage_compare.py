#!/usr/bin/env python3
"""Registers, LDS, scratch and occupancy of the decode kernels, of k_index and of the encoder's kernels in two source
trees, instantiation by instantiation: the compiler remarks libaec_amd/csrc/resusage.sh prints (-Rpass-analysis=kernel-resource-usage), with the
template arguments kept -- resusage.sh folds them -- so that every existing instantiation can be found again in a tree
that adds a template flag.
    python tests/resusage_compare.py <parent tree>/libaec_amd/csrc <this tree>/libaec_amd/csrc
The CHUNKS flag (the last template argument of k_decode, k_decode_wave and k_decode_redo) is dropped from the names of
the second tree where it is false; instantiations where it is true are listed as new."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
UNITS = [("aec_dec.hip (no part)", "aec_dec.hip", [])] + \
        [(f"aec_dec.hip -DAEC_DEC_PART={p}", "aec_dec.hip", [f"-DAEC_DEC_PART={p}"]) for p in (0, 8, 16, 32, 64)] + \
        [("aec_idx.hip (k_index)", "aec_idx.hip", [])] + \
        [("aec_enc.hip (no part)", "aec_enc.hip", [])] + \
        [(f"aec_enc.hip -DAEC_ENC_PART={p}", "aec_enc.hip", [f"-DAEC_ENC_PART={p}"]) for p in (0, 8, 16, 32, 64)]
KEYS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]"]
FLAG_AT = {"k_decode": 7, "k_decode_wave": 4, "k_decode_redo": 3}


def remarks(csrc, src, defs):
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", *defs, "-c", src, "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], cwd=csrc, capture_output=True, text=True)
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+(" + "|".join(re.escape(k) for k in KEYS) + r"): (\d+)", line)
        if m and cur:
            out[cur][m.group(1)] = int(m.group(2))
    names = list(out)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return {short(p): out[n] for n, p in zip(names, plain)}


def short(d):
    """kernel name and template arguments, without namespaces and parameter list"""
    d = re.sub(r"^void ", "", d).replace("aec::(anonymous namespace)::", "").replace("aec::", "")
    depth = 0
    for i, ch in enumerate(d):
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            return d[:i]
    return d


def without_flag(name):
    m = re.match(r"(k_decode|k_decode_wave|k_decode_redo)<(.*)>$", name)
    if not m:
        return name, False
    args = [a.strip() for a in m.group(2).split(",")]
    if len(args) == FLAG_AT[m.group(1)]:
        if args[-1] == "true":
            return name, True
        args = args[:-1]
    return f"{m.group(1)}<{', '.join(args)}>", False


def main():
    parent, branch = sys.argv[1], sys.argv[2]
    with ThreadPoolExecutor(max_workers=8) as ex:
        jobs = [(ex.submit(remarks, parent, src, defs), ex.submit(remarks, branch, src, defs)) for _, src, defs in UNITS]
    same = changed = 0
    fmt = lambda v: " ".join(f"{v[k]:5d}" for k in KEYS)      # noqa: E731
    print("columns: sgpr vgpr agpr scratch(bytes/lane) lds(bytes/block, static) occupancy(waves/SIMD)")
    for (title, src, _), (jp, jb) in zip(UNITS, jobs):
        P, B, new = jp.result(), {}, {}
        for name, v in jb.result().items():
            plain, is_new = without_flag(name)
            (new if is_new else B)[plain] = v
        if src == "aec_idx.hip":
            P, B = ({k: v for k, v in t.items() if k == "k_index"} for t in (P, B))
        print(f"== {title}")
        for name in sorted(set(P) | set(B)):
            a, b = P.get(name), B.get(name)
            if a == b:
                same += 1
                print(f"  same     {name:56s} {fmt(a)}")
            elif a is None:
                print(f"  new      {name:56s} {fmt(b)}")
            else:
                changed += 1
                print(f"  CHANGED  {name:56s} parent {fmt(a)} | branch {fmt(b) if b else 'gone'}")
        for name in sorted(new):
            print(f"  new      {name:56s} {fmt(new[name])}")
    print(f"existing instantiations with the same figures: {same}; changed or gone: {changed}")


if __name__ == "__main__":
    main()
