"""CPU check of the arithmetic of aec_gpu_sz_estimate_async (libaec_amd/csrc/aec_szest.h) through the host harness
tests/emul/sz_est_emul.cpp, which runs it wavefront by wavefront and lane by lane as the kernels of aec_szest.hip do: per
chunk and per pixels-per-block, the bits must be the oracle's total_bits of the padded coder input that py_layout + NumPy
padding build, and their bytes the length of the stream the reference's shim made (tests/golden/sz_estimate.json)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import sz_estimate_cases as sc
from helpers import ROOT
from test_sz_layout import py_layout

EMUL_DIR = os.path.join(ROOT, "tests", "emul")
EMUL_SRC = os.path.join(EMUL_DIR, "sz_est_emul.cpp")
EMUL_SO = os.path.join(EMUL_DIR, "_build", "libsz_est_emul.so")
NOT_ASKED = (1 << 64) - 1


@pytest.fixture(scope="module")
def emul():
    os.makedirs(os.path.dirname(EMUL_SO), exist_ok=True)
    srcs = [EMUL_SRC] + [os.path.join(ROOT, "libaec_amd", "csrc", h) for h in
                         ("aec_szest.h", "aec_est.h", "aec_szmap.h", "aec_lane.h", "aec_cfg.h")]
    if not os.path.exists(EMUL_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMUL_SO) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", EMUL_SO, EMUL_SRC], check=True)
    lib = C.CDLL(EMUL_SO)
    lib.sz_est_emul.restype = C.c_int
    return lib


def vp(a):
    return C.c_void_p(a.ctypes.data)


def run_emul(lib, opts, bpp, pps, chunks, how="aligned", skew=0, force_generic=0):
    buf, offs, sizes = sc.place(chunks, how, skew)
    n = len(chunks)
    bits = np.zeros(max(1, 4 * n), dtype=np.uint64)
    paths = np.full(max(1, n), 99, dtype=np.uint32)
    total = (C.c_uint64 * 4)()
    best, passes, pieces = C.c_uint32(99), C.c_uint32(99), C.c_uint64(0)
    rc = lib.sz_est_emul((C.c_int * 2)(opts, bpp), (C.c_uint * 4)(*pps), C.c_uint32(skew), vp(buf), C.c_uint64(buf.size), vp(offs),
                         vp(sizes), C.c_uint64(n), C.c_int(force_generic), vp(bits), total, C.byref(best), C.byref(passes),
                         C.byref(pieces), vp(paths))
    return dict(rc=rc, bits=[[int(v) for v in bits[4 * c:4 * c + 4]] for c in range(n)], total=[int(v) for v in total],
                best=best.value, passes=passes.value, pieces=pieces.value, paths=[int(v) for v in paths[:n]])


def expected(name, opts, bpp, pps, chunks):
    """(bits per chunk and size, total_bytes, best, passes, pieces) by the oracle and the restated layout"""
    bits = [sc.oracle_bits(opts, bpp, pps, c) for c in chunks]
    total = [NOT_ASKED] * 4
    for i in sc.asked(pps):
        total[i] = sum(max(1, (b[i] + 7) // 8) for b in bits)
    best = min(sc.asked(pps), key=lambda i: (total[i], i))
    pieces = 0
    for line in set(p for p in pps if p):
        i = [k for k in range(4) if pps[k] == line][0]
        pieces += sum(py_layout(opts, bpp, 8 << i, line, c.size)["lines"] for c in chunks) * (-(-line // 64))
    return bits, total, best, len(set(p for p in pps if p)), pieces


GROUPS = sorted(set(c[0].split("-")[0] for c in sc.all_cases()), key=lambda g: (not g.isdigit(), int(g) if g.isdigit() else 0, g))


@pytest.mark.parametrize("group", GROUPS)
def test_bits_are_the_oracles_and_bytes_the_reference_shims(emul, group):
    golden = sc.golden()
    for name, opts, bpp, pps, chunks in sc.all_cases():
        if name.split("-")[0] != group:
            continue
        if name == "small-300":
            chunks = chunks[::12]                                       # (the GPU test takes all of them)
        bits, total, best, passes, pieces = expected(name, opts, bpp, pps, chunks)
        got = run_emul(emul, opts, bpp, pps, chunks)
        assert got["rc"] == 0, name
        for c in range(len(chunks)):
            want = [b if b is not None else NOT_ASKED for b in bits[c]]
            assert got["bits"][c] == want, (name, c, chunks[c].size)
            ref = golden[name][12 * c if name == "small-300" else c]
            assert [max(1, (b + 7) // 8) if b is not None else None for b in bits[c]] == ref, (name, c)
        assert (got["total"], got["best"], got["passes"], got["pieces"]) == (total, best, passes, pieces), name
        # the same through the byte-wise map alone, and with the chunks at odd offsets in another order
        for kw in (dict(force_generic=1), dict(how="shuffled", skew=5)):
            other = run_emul(emul, opts, bpp, pps, chunks, **kw)
            assert (other["rc"], other["bits"], other["total"], other["best"]) == (0, got["bits"], got["total"], got["best"]), (name, kw)


def test_every_path_serves_chunks_of_the_cases(emul):
    """generic, straight and 4-byte planes: chunks at 16-byte boundaries take the fast path their scan line allows"""
    by_name = {c[0]: c for c in sc.all_cases()}
    for name, want in (("64-16bpp-nn", {1}), ("64-32bpp-nn", {0, 2}), ("65-8bpp-nn", {0}), ("mixed-32", {0, 2}), ("32768-8bpp-zero", {1})):
        _, opts, bpp, pps, chunks = by_name[name]
        assert set(run_emul(emul, opts, bpp, pps, chunks)["paths"]) == want, name
        assert set(run_emul(emul, opts, bpp, pps, chunks, "shuffled", 5)["paths"]) <= {0, 1, 2}


def test_one_eligible_chunk_between_two_odd_ones(emul):
    """both fast paths and the byte-wise map in one call, chunk by chunk"""
    rng = np.random.default_rng(3)
    for bpp, pps, want in ((32, 64, [0, 2, 0]), (16, 64, [0, 1, 0])):
        opts = sc.NN | sc.RAW
        chunks = [sc.pixels(rng, "walk", 2 * pps, bpp, opts) for _ in range(3)]
        buf, offs, sizes = sc.place(chunks, "aligned")
        got = run_emul(emul, opts, bpp, [pps] * 4, chunks)
        assert got["paths"] == [want[1]] * 3
        # chunks 0 and 2 off a boundary, the middle one on it
        n = int(sizes[0])
        mid = 16 * (-(-(3 + n) // 16))
        layout = np.array([3, mid, mid + n + 5], dtype=np.uint64)
        buf = np.full(mid + 2 * n + 5 + 16, 0x3C, dtype=np.uint8)
        for o, c in zip(layout, chunks):
            buf[int(o):int(o) + c.size] = c
        bits = np.zeros(12, dtype=np.uint64)
        paths = np.zeros(3, dtype=np.uint32)
        total = (C.c_uint64 * 4)()
        best, passes, pieces = C.c_uint32(), C.c_uint32(), C.c_uint64()
        rc = emul.sz_est_emul((C.c_int * 2)(opts, bpp), (C.c_uint * 4)(*[pps] * 4), C.c_uint32(0), vp(buf), C.c_uint64(buf.size),
                              vp(layout), vp(sizes), C.c_uint64(3), C.c_int(0), vp(bits), total, C.byref(best), C.byref(passes),
                              C.byref(pieces), vp(paths))
        assert rc == 0 and [int(p) for p in paths] == want
        assert [[int(v) for v in bits[4 * c:4 * c + 4]] for c in range(3)] == got["bits"]


def test_refusals(emul):
    one = [np.zeros(64, dtype=np.uint8)]
    assert run_emul(emul, sc.NN, 8, [0, 0, 0, 0], one)["rc"] == -1                   # no size asked
    assert run_emul(emul, sc.NN, 8, [32769, 0, 0, 0], one)["rc"] == -1               # 4097 blocks of 8 per line
    assert run_emul(emul, sc.NN, 8, [0, 32769, 0, 0], one)["rc"] == 0                # ... but 2049 of 16
    assert run_emul(emul, sc.NN, 33, [64] * 4, one)["rc"] == -1
    assert run_emul(emul, sc.NN, 64, [64] * 4, [np.zeros(7, dtype=np.uint8)])["rc"] == -1    # no whole pixel
    got = run_emul(emul, sc.NN, 8, [64, 0, 64, 0], [])                               # an empty batch is taken
    assert (got["rc"], got["total"], got["best"], got["pieces"]) == (0, [0, NOT_ASKED, 0, NOT_ASKED], 0, 0)


def test_stand_alone_program_under_asan_and_ubsan_gives_the_same(emul, tmp_path):
    exe, path = str(tmp_path / "sz_est_emul"), str(tmp_path / "cases.bin")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wno-unknown-pragmas", "-DSZ_EST_EMUL_MAIN", "-o", exe, EMUL_SRC], check=True)
    want = []
    with open(path, "wb") as f:
        for name, opts, bpp, pps, chunks in sc.all_cases():
            if name == "small-300":
                chunks = chunks[::12]
            for how, skew, force in (("aligned", 0, 0), ("shuffled", 5, 0)):
                buf, offs, sizes = sc.place(chunks, how, skew)
                f.write(struct.pack("<2i6I2Q", opts, bpp, *pps, skew, force, len(chunks), buf.size))
                f.write(offs.tobytes() + sizes.tobytes() + buf.tobytes())
                got = run_emul(emul, opts, bpp, pps, chunks, how, skew, force)
                want.append(" ".join(str(v) for v in [got["rc"], got["passes"], got["pieces"], got["best"], "|"] + got["total"] + ["|"] +
                                     [b for row in got["bits"] for b in row]))
    run = subprocess.run([exe, path], capture_output=True, text=True)
    lines = run.stdout.strip().split("\n")
    assert run.returncode == 0 and lines[-1] == f"{len(want)} cases ok", run.stdout[-2000:] + run.stderr[-4000:]
    assert [l.strip() for l in lines[:-1]] == want
