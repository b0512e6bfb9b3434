"""SZIP chunks of any size in one call, the part that needs no device: the plan (aec_gpu_sz_chunks_plan, host arithmetic in
libaec.so.0) and the per-chunk index arithmetic of libaec_amd/csrc/aec_szmap.h (SzChunk), which
tests/emul/sz_chunks_emul.cpp runs wavefront by wavefront and lane by lane as the kernels of aec_sz.hip do: against the
NumPy restatement of sz_abi.cpp per chunk, and against streams the reference's shim made
(tests/golden/sz_chunks_vectors.npz)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers
from sz_chunks_cases import eligible, golden_batches, size_list, synthetic_batch
from test_sz_layout import MSB, NN, RAW, SYNTHETIC, np_marshal, np_unmarshal, prm, py_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
EMUL_SO = os.path.join(EMUL_DIR, "_build", "libsz_chunks_emul.so")
# SzChunk of aec_szmap.h
DESC = np.dtype([("off", "<u8"), ("chunk_bytes", "<u8"), ("work_off", "<u8"), ("coded_bytes", "<u8"), ("pixels", "<u8"),
                 ("lines", "<u8"), ("coder_bytes", "<u8"), ("wave0", "<u8", 2), ("planes", "<u4"), ("head", "<u4")])
FILL = 0xA5


@pytest.fixture(scope="module")
def emul():
    os.makedirs(os.path.dirname(EMUL_SO), exist_ok=True)
    srcs = [os.path.join(EMUL_DIR, "sz_chunks_emul.cpp")] + [os.path.join(ROOT, "libaec_amd", "csrc", h) for h in
                                                              ("aec_szmap.h", "aec_cfg.h", "aec_lane.h")]
    if not os.path.exists(EMUL_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMUL_SO) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"),
                        "-o", EMUL_SO, srcs[0]], check=True)
    lib = C.CDLL(EMUL_SO)
    lib.emul_szc_make.restype = C.c_int
    lib.emul_szc_table.restype = None
    lib.emul_szc_marshal.restype = C.c_int64
    lib.emul_szc_unmarshal.restype = C.c_int64
    return lib


@pytest.fixture(scope="module")
def szgpu():
    import __graft_entry__ as g
    g.build()
    from libaec_amd import szgpu as s
    return s


def up16(v):
    return (v + 15) // 16 * 16


def vp(a):
    return C.c_void_p(a.ctypes.data)


def make(emul, params, base_low, offsets, sizes, unmarshal):
    """the descriptors (n + 1 records) and the wavefront table of a batch, or None where it is refused"""
    offsets, sizes = np.asarray(offsets, dtype=np.uint64), np.asarray(sizes, dtype=np.uint64)
    desc = np.zeros(sizes.size + 1, dtype=DESC)
    assert DESC.itemsize == 80
    if emul.emul_szc_make(prm(*params), C.c_uint32(base_low), vp(offsets), vp(sizes), C.c_uint64(sizes.size), C.c_int(unmarshal),
                          vp(desc)) != 0:
        return None
    table = np.full(int(desc[-1]["wave0"].sum()) + 1, 0xFFFFFFFF, dtype=np.uint32)
    emul.emul_szc_table(vp(desc), C.c_uint64(sizes.size), vp(table))
    assert table[-1] == 0xFFFFFFFF
    return desc, table[:-1]


def place(sizes, skew, share=False):
    """offsets of chunks in a buffer whose byte 0 is `skew` off a 16-byte boundary: chunks 0 and 1 back to back (with
    share, they share a 16-byte line whatever their sizes), the others after gaps of 3, 16, 29, ... bytes"""
    offs, at = [], 0
    for i, s in enumerate(sizes):
        offs.append(at)
        at += s + (0 if i == 0 and share else 3 + 13 * i)
    return offs, at


def emul_marshal(emul, params, chunks, skew):
    sizes = [c.size for c in chunks]
    offs, total = place(sizes, skew)
    src = np.full(total, FILL, dtype=np.uint8)
    for o, c in zip(offs, chunks):
        src[o:o + c.size] = c
    desc, table = make(emul, params, skew, offs, sizes, 0)
    work = np.full(int(desc[-1]["work_off"]) + 32, FILL, dtype=np.uint8)
    straight = C.c_uint64()
    differ = emul.emul_szc_marshal(prm(*params), C.c_uint32(skew), vp(desc), C.c_uint64(len(sizes)), vp(table), vp(src), vp(work),
                                   C.byref(straight))
    assert differ == 0, f"the cursor's walk and the map differ at {differ} bytes"
    return desc, work, straight.value


# ---- the plan -----------------------------------------------------------------------------------------------------------
def py_plan(params, sizes):
    Ls = [py_layout(*params, s) for s in sizes]
    if any(L is None for L in Ls):
        return None
    offs = np.cumsum([0] + [up16(L["coder_bytes"]) for L in Ls])
    return dict(work_offsets=[int(v) for v in offs[:-1]], work_bytes=int(offs[-1]), rsi_entries=sum(L["lines"] + 1 for L in Ls),
                direct=int(all(L["passthrough"] for L in Ls)), coder_bytes=[L["coder_bytes"] for L in Ls], L=Ls[0])


def test_plan_against_its_restatement(szgpu):
    from libaec_amd import gpu
    batches = [(c[:4], size_list(c)) for c in SYNTHETIC] + [(p, s) for _, p, s, _, _ in golden_batches()]
    batches.append(((NN | RAW, 8, 8, 1024), [4096, 1024, 65536]))                       # every chunk is the coder's input
    batches.append(((NN | RAW, 8, 8, 1024), [4096, 1000]))                              # ... but one
    seen = 0
    for params, sizes in batches:
        want, got = py_plan(params, sizes), szgpu.chunks_plan(*params, sizes)
        assert want is not None and got is not None, (params, sizes)
        assert [int(v) for v in got["work_offsets"]] == want["work_offsets"]
        assert (got["work_bytes"], got["rsi_entries"], got["direct"]) == (want["work_bytes"], want["rsi_entries"], want["direct"])
        L = want["L"]
        assert got["coder"] == (L["bps"], L["bs"], L["rsi"], L["flags"])
        coder = gpu.encode_chunks_plan(L["bps"], L["bs"], L["rsi"], L["flags"], np.array(want["coder_bytes"], dtype=np.uint64))
        assert got["out_bound"] == coder["out_bound"] and got["rsi_entries"] == coder["rsi_entries"]
        assert got["workspace_bytes"] > coder["workspace_bytes"]
        seen += got["direct"]
    assert seen == 2                                                                     # (beyond-128 and the first of the two)


def test_plan_refusals(szgpu):
    lib = szgpu._lib()
    assert szgpu.chunks_plan(NN | RAW, 16, 16, 100, [200, 1, 200]) is None              # a chunk without a whole pixel
    assert szgpu.chunks_plan(NN | RAW, 64, 8, 24, [800, 7]) is None
    assert szgpu.chunks_plan(NN | RAW, 16, 15, 100, [200]) is None                      # an SZ_com_t the layout rejects
    assert szgpu.chunks_plan(NN | RAW, 33, 16, 100, [200]) is None
    assert szgpu.chunks_plan(NN | RAW, 8, 8, 1024, [1 << 35]) is None                   # a chunk no launch can count
    sizes = np.array([200, 400], dtype=np.uint64)
    p = szgpu.SZ_com_t(NN | RAW, 16, 16, 100)
    assert lib.aec_gpu_sz_chunks_plan(C.byref(p), vp(sizes), 2, None, None) == 0        # no plan to fill
    plan = szgpu.ChunksPlan()
    assert lib.aec_gpu_sz_chunks_plan(None, vp(sizes), 2, C.byref(plan), None) == 0
    assert lib.aec_gpu_sz_chunks_plan(C.byref(p), None, 2, C.byref(plan), None) == 0
    assert lib.aec_gpu_sz_chunks_plan(C.byref(p), vp(sizes), 2, C.byref(plan), None) == 1  # (work_offsets is optional)
    assert szgpu.chunks_plan(NN | RAW, 16, 16, 100, [])["work_bytes"] == 0              # an empty batch is taken


# ---- the maps over unequal batches ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SYNTHETIC, ids=lambda c: f"{c[1]}bpp-{c[2]}-{c[3]}")
def test_maps_on_unequal_batches(emul, case):
    params = case[:4]
    sizes, chunks = synthetic_batch(case, seed=1)
    assert sizes[0] == py_layout(*params, 64)["word"] or sizes[0] == py_layout(*params, 64)["pixel"]
    assert sizes[1] == case[4] and py_layout(*params, sizes[2])["coded_bytes"] % py_layout(*params, sizes[2])["line"] == 0
    assert eligible(case, sizes[2]) == (case[1] in (32, 64))
    assert py_layout(*params, sizes[-1])["lines"] == 1 and py_layout(*params, sizes[-1])["coded_bytes"] < py_layout(*params, 64)["line"]
    if len(sizes) == 5:
        assert py_layout(*params, sizes[3])["coded_bytes"] < sizes[3]
    want = [np_marshal(c, *params) for c in chunks]
    for skew in (0, 5):
        desc, work, straight = emul_marshal(emul, params, chunks, skew)
        assert int(desc[-1]["work_off"]) == sum(up16(w.size) for w in want)
        written = np.zeros(work.size, dtype=bool)
        for i, w in enumerate(want):
            o = int(desc[i]["work_off"])
            assert o % 16 == 0 and np.array_equal(work[o:o + w.size], w), (skew, i)
            written[o:o + w.size] = True
        assert np.all(work[~written] == FILL), skew                       # the gaps between rooms and all behind the last
        # (chunk 2 of a set with planes lies at offset sizes[0] + sizes[1] + ...: whether it is aligned decides its path)
        for i, s in enumerate(sizes):
            aligned = (skew + int(desc[i]["off"])) % 16 == 0
            assert int(desc[i]["planes"]) == int(eligible(case, s) and aligned), (skew, i)
    # and back: heads 0 and 11, chunks 0 and 1 sharing a 16-byte line
    work = np.full(sum(up16(w.size) for w in want) + 32, FILL, dtype=np.uint8)
    at = 0
    for w in want:
        work[at:at + w.size] = w
        at += up16(w.size)
    for head in (0, 11):
        offs, total = place(sizes, head, share=True)
        assert (head + offs[1]) // 16 == (head + offs[1] - 1) // 16                  # (they do share one)
        desc, table = make(emul, params, head, offs, sizes, 1)
        assert int(desc[0]["head"]) == head
        dst = np.full(total, FILL, dtype=np.uint8)
        straight = C.c_uint64()
        twice = emul.emul_szc_unmarshal(prm(*params), C.c_uint32(head), vp(desc), C.c_uint64(len(sizes)), vp(table), vp(work), vp(dst),
                                        C.c_uint64(total), C.byref(straight))
        assert twice == 0
        written = np.zeros(total, dtype=bool)
        for i, (o, c) in enumerate(zip(offs, chunks)):
            assert np.array_equal(dst[o:o + c.size], np_unmarshal(want[i], *params, c.size)), (head, i)
            L = py_layout(*params, c.size)
            assert np.array_equal(dst[o:o + L["coded_bytes"]], c[:L["coded_bytes"]]) and not dst[o + L["coded_bytes"]:o + c.size].any()
            written[o:o + c.size] = True
        assert np.all(dst[~written] == FILL), head


# ---- the wavefront table ------------------------------------------------------------------------------------------------------
def test_wavefront_table_against_a_search(emul):
    """32 / 16 / 1024: chunks smaller than one wavefront's 1 KiB, a chunk of exactly 64 groups, eligible and ineligible
    chunks alternating"""
    params = (NN | RAW, 32, 16, 1024)
    sizes = [4, 1024, 8192, 4004, 64, 16384, 12, 4096 + 4, 4096, 1028, 32768]
    case = params + (0,)
    offs, at = [], 0
    for s in sizes:
        offs.append(at)
        at += up16(s)
    for unmarshal, skew in ((0, 0), (1, 0), (0, 8), (1, 8)):
        desc, table = make(emul, params, skew, offs, sizes, unmarshal)
        nb, np_ = (int(v) for v in desc[-1]["wave0"])
        assert table.size == nb + np_
        want = [[], []]
        for i, s in enumerate(sizes):
            L = py_layout(*params, s)
            planes = eligible(case, s) and skew == 0
            assert int(desc[i]["planes"]) == int(planes)
            if planes:
                waves = -(-(s // 16) // 64)
            elif unmarshal:
                waves = -(-((skew + s + 15) // 16) // 64)
            else:
                waves = -(-((L["coder_bytes"] + 15) // 16) // 64)
            assert int(desc[i]["wave0"][int(planes)]) == len(want[int(planes)])
            want[int(planes)] += [i] * waves
        assert [int(v) for v in table] == want[0] + want[1], (unmarshal, skew)
        if skew == 0:
            assert nb and np_ and py_layout(*params, sizes[1])["coder_bytes"] == 64 * 16
            planes = [int(v) for v in desc[:-1]["planes"]]
            assert planes[1:6] == [1, 1, 0, 1, 1] and planes[6:9] == [0, 0, 1]


# ---- against the reference's own streams ------------------------------------------------------------------------------------------
def test_marshal_then_oracle_encoder_gives_the_reference_shims_streams(emul):
    seen = 0
    for name, params, sizes, chunks, streams in golden_batches():
        L = py_layout(*params, 64)
        desc, work, _ = emul_marshal(emul, params, chunks, 0)
        step = max(1, len(sizes) // 12)                                   # (of the 300 small chunks: every 25th)
        for i in range(0, len(sizes), step):
            o, n = int(desc[i]["work_off"]), int(desc[i]["coder_bytes"])
            rc, enc, _, _, _ = helpers.oracle_encode(work[o:o + n], L["bps"], L["bs"], L["rsi"], L["flags"])
            assert rc == helpers.AEC_OK and enc == streams[i], (name, i)
            seen += 1
    assert seen >= 40


# ---- the emulation under the sanitizers -------------------------------------------------------------------------------------------
def test_emulation_as_a_stand_alone_program_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "sz_chunks_emul")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wno-unknown-pragmas", "-DSZ_CHUNKS_EMUL_MAIN", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(EMUL_DIR, "sz_chunks_emul.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr
