"""SZIP chunks on the device, the part that needs none: the layout (aec_gpu_sz_layout, host arithmetic in libaec.so.0) and
the index arithmetic of libaec_amd/csrc/aec_szmap.h, which tests/emul/sz_emul.cpp runs lane by lane as the kernels of
aec_sz.hip do.  Pinned to data the reference's shim made (tests/golden/sz_vectors.npz: marshal + oracle encoder must give
the stored stream, oracle decoder + un-marshal the stored input) and to a NumPy restatement of sz_abi.cpp's
prepare_compress / finish_decompress (reference src/sz_compat.c:39-108, 134-166, 208-261)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers
from conftest import GOLDEN_DIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
EMUL_SO = os.path.join(EMUL_DIR, "_build", "libsz_emul.so")
MSB, NN, RAW = 16, 32, 128          # SZ_MSB_OPTION_MASK, SZ_NN_OPTION_MASK, SZ_RAW_OPTION_MASK


@pytest.fixture(scope="module")
def emul():
    os.makedirs(os.path.dirname(EMUL_SO), exist_ok=True)
    srcs = [os.path.join(EMUL_DIR, "sz_emul.cpp")] + [os.path.join(ROOT, "libaec_amd", "csrc", h) for h in
                                                       ("aec_szmap.h", "aec_cfg.h", "aec_lane.h")]
    if not os.path.exists(EMUL_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMUL_SO) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"),
                        "-o", EMUL_SO, srcs[0]], check=True)
    lib = C.CDLL(EMUL_SO)
    lib.emul_sz_layout.restype = C.c_int
    lib.emul_sz_marshal.restype = C.c_int64
    lib.emul_sz_unmarshal.restype = C.c_int64
    lib.emul_sz_planes.restype = C.c_int
    return lib


@pytest.fixture(scope="module")
def szgpu():
    import __graft_entry__ as g
    g.build()
    from libaec_amd import szgpu as s
    return s


# ---- restatements ----------------------------------------------------------------------------------------------------
def py_layout(opts, bpp, ppb, pps, chunk_bytes):
    """what aec_gpu_sz_layout must say, or None where it must refuse"""
    if ppb <= 0 or ppb % 2 or ppb > 64 or pps <= 0 or bpp <= 0:
        return None
    planes = bpp in (32, 64)
    bps = 8 if planes else bpp
    if bps > 32:
        return None
    rsi = -(-pps // ppb)
    if rsi > 4096:
        return None
    pixel = 4 if bps > 16 else (2 if bps > 8 else 1)
    flags = helpers.AEC_NOT_ENFORCE | (helpers.AEC_DATA_MSB if opts & MSB else 0) | (helpers.AEC_DATA_PREPROCESS if opts & NN else 0)
    coded = chunk_bytes - chunk_bytes % (bpp // 8 if planes else pixel)
    if coded == 0:
        return None
    line, padded = pps * pixel, rsi * ppb * pixel
    lines = -(-coded // line)
    return dict(bps=bps, bs=ppb, rsi=rsi, flags=flags, word=bpp // 8 if planes else 0, pixel=pixel, repeat=int(bool(opts & NN)),
                passthrough=int(not planes and padded == line and coded % line == 0 and coded == chunk_bytes),
                line=line, padded_line=padded, lines=lines, coder_bytes=lines * padded, coded_bytes=coded)


def np_marshal(chunk, opts, bpp, ppb, pps):
    """prepare_compress of sz_abi.cpp on one chunk: the bytes the coder is given"""
    L = py_layout(opts, bpp, ppb, pps, chunk.size)
    src = chunk[:L["coded_bytes"]]
    if L["word"]:
        src = src.reshape(-1, L["word"]).T.reshape(-1)                    # to_planes
    out = np.zeros((L["lines"], L["padded_line"]), dtype=np.uint8)
    for l in range(L["lines"]):
        row = src[l * L["line"]:(l + 1) * L["line"]]
        out[l, :row.size] = row
        if L["repeat"] and row.size < L["padded_line"]:
            out[l, row.size:] = np.tile(row[-L["pixel"]:], (L["padded_line"] - row.size) // L["pixel"])
    return out.reshape(-1)


def np_unmarshal(coder_out, opts, bpp, ppb, pps, chunk_bytes):
    """finish_decompress of sz_abi.cpp; the trailing fraction of a pixel, which is never coded, is zero"""
    L = py_layout(opts, bpp, ppb, pps, chunk_bytes)
    flat = coder_out.reshape(L["lines"], L["padded_line"])[:, :L["line"]].reshape(-1)[:L["coded_bytes"]]
    if L["word"]:
        flat = flat.reshape(L["word"], -1).T.reshape(-1)                  # from_planes
    out = np.zeros(chunk_bytes, dtype=np.uint8)
    out[:L["coded_bytes"]] = flat
    return out


def prm(opts, bpp, ppb, pps):
    return (C.c_int * 4)(opts, bpp, ppb, pps)


def emul_marshal(emul, chunks, opts, bpp, ppb, pps, head=0):
    data = np.ascontiguousarray(chunks).reshape(-1)
    n, chunk_bytes = chunks.shape
    L = py_layout(opts, bpp, ppb, pps, chunk_bytes)
    out = np.full(n * L["coder_bytes"], 0xA5, dtype=np.uint8)
    straight = C.c_uint64()
    differ = emul.emul_sz_marshal(prm(opts, bpp, ppb, pps), C.c_uint64(chunk_bytes), C.c_uint64(n), C.c_void_p(data.ctypes.data),
                                  C.c_void_p(out.ctypes.data), C.c_uint32(head), C.byref(straight))
    assert differ == 0, f"the cursor's walk and the map differ at {differ} bytes"
    return out.reshape(n, -1), straight.value


def emul_unmarshal(emul, coder_out, opts, bpp, ppb, pps, chunk_bytes, head=0):
    data = np.ascontiguousarray(coder_out).reshape(-1)
    n = coder_out.shape[0]
    dst = np.full(n * chunk_bytes, 0xA5, dtype=np.uint8)
    straight = C.c_uint64()
    rc = emul.emul_sz_unmarshal(prm(opts, bpp, ppb, pps), C.c_uint64(chunk_bytes), C.c_uint64(n), C.c_void_p(data.ctypes.data),
                                C.c_void_p(dst.ctypes.data), C.c_uint32(head), C.byref(straight))
    assert rc == 0
    return dst.reshape(n, -1), straight.value


def golden():
    z = np.load(os.path.join(GOLDEN_DIR, "sz_vectors.npz"))
    for i, name in enumerate(z["names"]):
        opts, bpp, ppb, pps = (int(v) for v in z["params"][i])
        data = z["inputs"][int(z["in_off"][i]):int(z["in_off"][i + 1])]
        comp = z["outputs"][int(z["out_off"][i]):int(z["out_off"][i + 1])].tobytes()
        yield str(name), opts, bpp, ppb, pps, data, comp


# the four synthetic chunks of the issue: (options, bits per pixel, pixels per block, pixels per scan line, chunk bytes)
SYNTHETIC = [
    (NN | RAW, 32, 16, 1000, 2501 * 4),          # lines straddle planes, partial last line, planes of odd length
    (NN | MSB | RAW, 64, 8, 24, 100 * 8),        # eight planes of 100 bytes under lines of 24
    (RAW, 8, 16, 100, 250),                      # zero fill
    (NN | RAW, 24, 32, 500, 1203 * 4),           # 24 bits in 4-byte containers
]


def synthetic_chunks(case, n, seed=0):
    opts, bpp, ppb, pps, chunk_bytes = case
    rng = np.random.default_rng(1000 * bpp + pps + seed)
    # (bytes that differ from their neighbours everywhere: a byte moved to the wrong place shows)
    data = rng.integers(0, 256, size=(n, chunk_bytes), dtype=np.uint8)
    if bpp not in (8, 16, 32, 64):
        # samples narrower than their container: the bits above bits-per-pixel are not coded, so they are zero here
        # (reference src/encode.c masks them on the way in; a round trip returns them as zero)
        unit = 4 if bpp > 16 else (2 if bpp > 8 else 1)
        px = data[:, :chunk_bytes // unit * unit].reshape(n, -1, unit)
        for b in range(unit):
            sig = unit - 1 - b if opts & MSB else b               # significance of byte b of the container
            px[:, :, b] &= np.uint8(max(0, min(255, (1 << max(0, bpp - 8 * sig)) - 1)))
    return data


# ---- layout -----------------------------------------------------------------------------------------------------------
def test_layout_against_its_restatement(emul, szgpu):
    seen = 0
    cases = [(o, b, p, s, d.size) for _, o, b, p, s, d, _ in golden()] + SYNTHETIC + [(NN, 16, 16, 1000, 2001), (NN, 32, 16, 1024, 4099)]
    assert len(list(golden())) == 9
    for opts, bpp, ppb, pps, size in cases:
        want = py_layout(opts, bpp, ppb, pps, size)
        got = szgpu.layout(opts, bpp, ppb, pps, size)
        assert got is not None and want is not None, (opts, bpp, ppb, pps, size)
        assert (got.coder.bits_per_sample, got.coder.block_size, got.coder.rsi, got.coder.flags) == \
               (want["bps"], want["bs"], want["rsi"], want["flags"])
        assert (got.word, got.pixel, got.fill_repeat, got.passthrough, got.line, got.padded_line, got.lines, got.coder_bytes,
                got.coded_bytes) == tuple(want[k] for k in ("word", "pixel", "repeat", "passthrough", "line", "padded_line",
                                                            "lines", "coder_bytes", "coded_bytes")), (opts, bpp, ppb, pps, size)
        out = np.zeros(13, dtype=np.uint64)
        assert emul.emul_sz_layout(prm(opts, bpp, ppb, pps), C.c_uint64(size), C.c_void_p(out.ctypes.data)) == 0
        assert [int(v) for v in out] == list(want.values())
        seen += want["passthrough"]
    assert seen >= 1                                                       # (the usual HDF5 chunk is among them)


@pytest.mark.parametrize("bpp,ppb,pps", [
    (8, 0, 100), (8, 7, 100), (8, 15, 100),          # pixels per block 0 or odd
    (8, 8, 0),                                       # pixels per scan line 0
    (0, 8, 100), (33, 8, 100), (48, 8, 100), (63, 8, 100), (65, 8, 100), (128, 8, 100),
    (8, 66, 660), (16, 128, 1024),                   # blocks beyond 64 pixels
])
def test_layout_refuses_what_the_host_path_refuses(emul, szgpu, bpp, ppb, pps):
    assert py_layout(NN, bpp, ppb, pps, 4096) is None
    assert szgpu.layout(NN, bpp, ppb, pps, 4096) is None                   # AEC_CONF_ERROR
    out = np.zeros(13, dtype=np.uint64)
    assert emul.emul_sz_layout(prm(NN, bpp, ppb, pps), C.c_uint64(4096), C.c_void_p(out.ctypes.data)) == helpers.AEC_CONF_ERROR
    assert szgpu.batch_ok(NN, bpp, ppb, pps, 4096, 4) == 0


# ---- the maps against the reference's own streams -----------------------------------------------------------------------
def test_marshal_then_oracle_encoder_gives_the_reference_shims_stream(emul):
    for name, opts, bpp, ppb, pps, data, comp in golden():
        L = py_layout(opts, bpp, ppb, pps, data.size)
        coder_in, _ = emul_marshal(emul, data.reshape(1, -1), opts, bpp, ppb, pps)
        assert np.array_equal(coder_in[0], np_marshal(data, opts, bpp, ppb, pps)), name
        rc, enc, _, _, _ = helpers.oracle_encode(coder_in[0], L["bps"], L["bs"], L["rsi"], L["flags"])
        assert rc == helpers.AEC_OK and enc == comp, name


def test_oracle_decoder_then_unmarshal_gives_the_input_back(emul):
    for name, opts, bpp, ppb, pps, data, comp in golden():
        L = py_layout(opts, bpp, ppb, pps, data.size)
        rc, dec, _ = helpers.oracle_decode(comp, L["bps"], L["bs"], L["rsi"], L["flags"] & ~helpers.AEC_NOT_ENFORCE, L["coder_bytes"])
        assert rc == helpers.AEC_OK and len(dec) == L["coder_bytes"], name
        back, _ = emul_unmarshal(emul, np.frombuffer(dec, dtype=np.uint8).reshape(1, -1), opts, bpp, ppb, pps, data.size)
        assert np.array_equal(back[0], data), name


# ---- the maps against the restatement of sz_abi.cpp ---------------------------------------------------------------------
@pytest.mark.parametrize("case", SYNTHETIC + [(NN | RAW, 8, 8, 1000, 1001), (NN | RAW, 16, 16, 1000, 6001), (NN | RAW, 8, 8, 1024, 4096)],
                         ids=lambda c: f"{c[1]}bpp-{c[2]}-{c[3]}-{c[4]}B")
def test_maps_on_batches_of_synthetic_chunks(emul, case):
    opts, bpp, ppb, pps, chunk_bytes = case
    chunks = synthetic_chunks(case, 3)
    want = np.stack([np_marshal(c, opts, bpp, ppb, pps) for c in chunks])
    for head in (0, 5):                                     # (groups cut differently: the same bytes)
        got, straight = emul_marshal(emul, chunks, opts, bpp, ppb, pps, head)
        assert np.array_equal(got, want), head
    want_back = np.stack([np_unmarshal(w, opts, bpp, ppb, pps, chunk_bytes) for w in want])
    L = py_layout(opts, bpp, ppb, pps, chunk_bytes)
    assert np.array_equal(want_back[:, :L["coded_bytes"]], chunks[:, :L["coded_bytes"]])       # (the restatement inverts itself)
    moved = {}
    for head in (0, 11):
        back, moved[head] = emul_unmarshal(emul, want, opts, bpp, ppb, pps, chunk_bytes, head)
        assert np.array_equal(back, want_back), head
    if not L["word"] and L["line"] >= 32:
        assert moved[0] > 0                                  # whole groups inside a line move as 16 bytes


@pytest.mark.parametrize("opts,bpp,ppb,pps,chunk_bytes,fast", [
    (NN | RAW, 32, 16, 1024, 16384, 1),          # whole lines, no padding at all
    (NN | MSB | RAW, 64, 8, 24, 800, 1),         # lines straddle the planes, a partial last line: k_sz_fill
    (RAW, 32, 16, 1000, 4000 * 4, 1),            # padded lines, zero fill
    (NN | RAW, 64, 10, 250, 64 * 8, 0),          # padded_line = 250: pieces would straddle lines
    (NN | RAW, 32, 16, 1000, 2501 * 4, 0),       # planes of odd length
])
def test_plane_lanes_transpose_in_registers(emul, opts, bpp, ppb, pps, chunk_bytes, fast):
    case = (opts, bpp, ppb, pps, chunk_bytes)
    chunks = synthetic_chunks(case, 3, seed=7)
    L = py_layout(*case)
    coder_in = np.full(3 * L["coder_bytes"], 0x5A, dtype=np.uint8)
    back = np.full(3 * chunk_bytes, 0x5A, dtype=np.uint8)
    data = np.ascontiguousarray(chunks).reshape(-1)
    rc = emul.emul_sz_planes(prm(opts, bpp, ppb, pps), C.c_uint64(chunk_bytes), C.c_uint64(3), C.c_void_p(data.ctypes.data),
                             C.c_void_p(coder_in.ctypes.data), C.c_void_p(back.ctypes.data))
    assert rc == fast
    if fast:
        want = np.stack([np_marshal(c, opts, bpp, ppb, pps) for c in chunks])
        assert np.array_equal(coder_in.reshape(3, -1), want)
        assert np.array_equal(back.reshape(3, -1), chunks)


# ---- the sweep of tests/test_gpu_sz_device.py draws cases the layout takes ----------------------------------------------
def test_the_gpu_sweeps_draws_are_mostly_valid(szgpu):
    from sz_device_cases import sweep_cases
    cases = list(sweep_cases())
    assert len(cases) == 30
    refused = sum(1 for c in cases if szgpu.layout(c["opts"], c["bpp"], c["ppb"], c["pps"], c["chunk_bytes"]) is None)
    assert refused * 4 <= len(cases), refused
    taken = [c for c in cases if szgpu.layout(c["opts"], c["bpp"], c["ppb"], c["pps"], c["chunk_bytes"]) is not None]
    assert {c["bpp"] for c in taken} >= {24, 32, 64} and any(c["bpp"] <= 8 for c in taken) and any(8 < c["bpp"] <= 16 for c in taken)
    assert all(1 <= c["n"] <= 12 and c["chunk_bytes"] <= 65536 for c in cases)
