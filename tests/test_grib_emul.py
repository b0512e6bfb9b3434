"""CPU check of the GRIB layer's arithmetic (libaec_amd/csrc/aec_grib.h) through the host harness tests/emul/grib_emul.cpp:
what k_grib_minmax does wavefront by wavefront, k_grib_params field by field and k_grib_quantise / k_grib_dequantise group
by group, against the NumPy model of tests/grib_cases.py bit for bit; and what the fixture tests/golden/grib_vectors.npz
must hold for the GPU tests to mean anything (the model's X, the contraction witnesses, the ties, an R that rounds down).

The model itself is checked against the contract restated in exact rationals (grib_cases.exact_R / exact_E / exact_x /
exact_y): on every value of grib_cases.edge_batches() and dequantise_cases() and on seeded random fields; the emulation
runs over those two lists as over the fixture's batches, and every case is asserted to sit on the threshold it names."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import grib_cases as gc
from helpers import ROOT, have_ref, ref_encode

EMUL_DIR = os.path.join(ROOT, "tests", "emul")
EMUL_SO = os.path.join(EMUL_DIR, "_build", "libgrib_emul.so")


@pytest.fixture(scope="module")
def emul():
    os.makedirs(os.path.dirname(EMUL_SO), exist_ok=True)
    srcs = [os.path.join(EMUL_DIR, "grib_emul.cpp")] + [os.path.join(ROOT, "libaec_amd", "csrc", h) for h in ("aec_grib.h", "aec_lane.h")]
    if not os.path.exists(EMUL_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMUL_SO) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", EMUL_SO,
                        srcs[0]], check=True)
    lib = C.CDLL(EMUL_SO)
    lib.grib_emul_pack.restype = C.c_int
    lib.grib_emul_unpack.restype = C.c_int
    lib.grib_emul_keys.restype = None
    return lib


@pytest.fixture(scope="module")
def golden():
    return gc.golden_batches()


def ptr(a):
    return C.c_void_p(a.ctypes.data)


def lay_out(b):
    """(source bytes with 0xA5 between the fields, offsets, work offsets, work bytes)"""
    offs, extent = gc.edge_placement(b)
    src = np.full(extent + 64, 0xA5, np.uint8)
    for o, f in zip(offs, b["fields"]):
        src[o:o + f.nbytes] = f.view(np.uint8)
    nbits, _, bs, _ = b["tmpl"]
    rooms = [gc.room(f.size, bs, nbits) for f in b["fields"]]
    work_offs = np.concatenate([[0], np.cumsum([gc.up16(r) for r in rooms])]).astype(np.uint64)
    return src, np.array(offs, np.uint64), work_offs, rooms


def given_records(b, model):
    rec = np.zeros(len(b["fields"]), gc.RECORD_DTYPE)
    for i, (R, E, st, x) in enumerate(model):
        rec[i] = (R, E, b["D"][i], 0)
    return rec


def run_pack(lib, b):
    src, offs, work_offs, rooms = lay_out(b)
    n = len(b["fields"])
    work = np.full(int(work_offs[-1]), 0x5A, np.uint8)
    fields = np.zeros(n, gc.RECORD_DTYPE)
    extremes = np.zeros(2 * n, np.uint64)
    n_values = np.array([f.size for f in b["fields"]], np.uint64)
    D = np.array(b["D"], np.int32)
    have = b["given"] is not None
    params = np.zeros(n, gc.RECORD_DTYPE)
    if have:
        for i, (R, E) in enumerate(b["given"]):
            params[i] = (R, E, b["D"][i], 0)
    rc = lib.grib_emul_pack((C.c_uint32 * 4)(*b["tmpl"]), b["elem"], ptr(src), ptr(offs), ptr(n_values), ptr(work_offs), ptr(D),
                            int(have), ptr(params), C.c_uint64(n), ptr(work), ptr(fields), ptr(extremes))
    assert rc == 0
    return fields, work, work_offs, rooms, extremes


def expected_work(b, model, work_offs, rooms, fill=0x5A):
    """the whole work buffer: the model's X in every room of a clean field, `fill` between the rooms; a mask of the bytes
    that are specified"""
    nbits = b["tmpl"][0]
    want = np.full(int(work_offs[-1]), fill, np.uint8)
    known = np.ones(want.size, bool)
    for (R, E, st, x), o, r in zip(model, work_offs, rooms):
        o = int(o)
        if x is None:
            known[o:o + r] = False
        else:
            want[o:o + r] = gc.x_bytes(x, nbits, r // gc.container(nbits))
    return want, known


BATCHES = [b["name"] for b in gc.batches()]


def check_pack(emul, b):
    """the emulated pack of a batch: records, the keys of the extremes and the whole work buffer are the model's"""
    name = b["name"]
    model = gc.model_of(b)
    fields, work, work_offs, rooms, extremes = run_pack(emul, b)
    for i, (R, E, st, x) in enumerate(model):
        assert int(fields[i]["status"]) == st and int(fields[i]["D"]) == b["D"][i], (name, i, fields[i], st)
        if st & gc.BAD:
            continue
        assert fields[i]["R"].tobytes() == np.float32(R).tobytes() and int(fields[i]["E"]) == E, (name, i, fields[i], R, E)
        f = b["fields"][i].astype(np.float64)
        lo, hi = f.min(), f.max()
        ends, k, back, k32, wide = np.array([lo, hi]), np.zeros(2, np.uint64), np.zeros(2), np.zeros(2, np.uint32), np.zeros(2, np.uint64)
        emul.grib_emul_keys(ptr(ends), C.c_uint64(2), ptr(k), ptr(back), ptr(k32), ptr(wide))
        if lo != 0 and hi != 0:             # (which zero a field's extreme is depends on the field)
            assert [int(v) for v in extremes[2 * i:2 * i + 2]] == [int(v) for v in k], (name, i)
    want, known = expected_work(b, model, work_offs, rooms)
    bad = np.flatnonzero((work != want) & known)
    assert bad.size == 0, (name, int(bad[0]), int(work[bad[0]]), int(want[bad[0]]))


def check_unpack(emul, b, model):
    """the emulated dequantise of the model's X under the model's parameters: the whole destination is the model's"""
    src, offs, work_offs, rooms = lay_out(b)
    want_work, known = expected_work(b, model, work_offs, rooms, fill=0xFF)
    n = len(b["fields"])
    n_values = np.array([f.size for f in b["fields"]], np.uint64)
    dst = np.full(src.size, 0xA5, np.uint8)
    params = given_records(b, model)
    rc = emul.grib_emul_unpack((C.c_uint32 * 4)(*b["tmpl"]), b["elem"], ptr(want_work), ptr(work_offs), ptr(n_values), ptr(params),
                               ptr(offs), C.c_uint64(n), ptr(dst))
    assert rc == 0
    want = np.full(src.size, 0xA5, np.uint8)
    skip = np.zeros(src.size, bool)
    for i, ((R, E, st, x), o, f) in enumerate(zip(model, offs, b["fields"])):
        o = int(o)
        if x is None:
            skip[o:o + f.nbytes] = True
            continue
        want[o:o + f.nbytes] = gc.dequantise(x, R, E, b["D"][i], b["dtype"]).view(np.uint8)
    bad = np.flatnonzero((dst != want) & ~skip)
    assert bad.size == 0, (b["name"], int(bad[0]))


@pytest.mark.parametrize("name", BATCHES)
def test_pack_is_the_models(emul, golden, name):
    check_pack(emul, next(g for g in golden if g["name"] == name))


@pytest.mark.parametrize("name", BATCHES)
def test_unpack_is_the_models(emul, golden, name):
    b = next(g for g in golden if g["name"] == name)
    check_unpack(emul, b, gc.model_of(b))


@pytest.mark.parametrize("name", [b["name"] for b in gc.extra_batches()])
def test_pack_of_the_extra_batches_is_the_models(emul, name):
    b = next(g for g in gc.extra_batches() if g["name"] == name)
    model = gc.model_of(b)
    fields, work, work_offs, rooms, extremes = run_pack(emul, b)
    assert [int(s) for s in fields["status"]] == [m[2] for m in model], name
    for f, (R, E, st, x) in zip(fields, model):
        if not st & gc.BAD:
            assert f["R"].tobytes() == np.float32(R).tobytes() and int(f["E"]) == E, name
    want, known = expected_work(b, model, work_offs, rooms)
    assert not ((work != want) & known).any(), name


def test_the_extra_batches_hold_what_they_are_for():
    given, wide = (gc.model_of(b) for b in gc.extra_batches())
    assert [m[2] for m in given] == [0, gc.BAD, 0]                      # bad and nothing else, under given parameters
    R, E, st, x = wide[0]
    assert E == 127 and st == gc.CLAMPED and int(x.max()) == 1 and wide[1][2] == 0


def test_nonfinite_fields_are_flagged_in_the_model(golden):
    """a NaN, an Inf and a NaN with the sign bit: the model flags exactly those three fields (what the device does with
    them, and that their neighbours stay exact, is tests/test_gpu_grib.py over the same batches)"""
    for name in ("nonfinite_f4", "nonfinite_f8"):
        b = next(g for g in golden if g["name"] == name)
        assert [m[2] & gc.BAD for m in gc.model_of(b)] == [0, 1, 0, 1, 0, 1]


def test_keys_keep_the_order_and_come_back(emul):
    v = np.array([-np.inf, -3.5e38, -1.5, -1e-310, -0.0, 0.0, 1e-310, 2.0 ** -130, 1.0, 1.0000000000000002, 3.5e38, np.inf])
    n = v.size
    k64, back, k32, wide = np.zeros(n, np.uint64), np.zeros(n), np.zeros(n, np.uint32), np.zeros(n, np.uint64)
    with np.errstate(over="ignore", under="ignore"):
        emul.grib_emul_keys(ptr(v), C.c_uint64(n), ptr(k64), ptr(back), ptr(k32), ptr(wide))
        f = v.astype(np.float32)
    assert np.all(np.diff(k64.astype(object)) > 0)
    assert back.tobytes() == v.tobytes()
    assert np.all(np.diff(k32.astype(object)) >= 0)
    k64f, f64, again = np.zeros(n, np.uint64), f.astype(np.float64), np.zeros(n, np.uint64)
    emul.grib_emul_keys(ptr(f64), C.c_uint64(n), ptr(k64f), ptr(back), ptr(k32), ptr(again))
    assert np.array_equal(wide, k64f)                      # widening a float's key = the key of the float as a double
    nan = np.array([np.nan, -np.nan])
    nan.view(np.uint64)[1] |= np.uint64(1 << 63)
    nan.view(np.uint64)[0] &= np.uint64((1 << 63) - 1)
    emul.grib_emul_keys(ptr(nan), C.c_uint64(2), ptr(k64), ptr(back), ptr(k32), ptr(wide))
    assert int(k64[0]) > int(k64f[-1]) and int(k64[1]) < int(k64f[0])       # NaNs sort to the ends


def test_the_fixture_holds_the_models_x(golden):
    for b in golden:
        for i, ((R, E, st, x), gx) in enumerate(zip(gc.model_of(b), b["X"])):
            assert (x is None) == (gx is None), (b["name"], i)
            if x is not None:
                assert np.array_equal(x, gx), (b["name"], i)
                assert int(x.max()) <= 2 ** b["tmpl"][0] - 1


def test_the_fixture_holds_the_generated_fields(golden):
    for b, g in zip(gc.batches(), golden):
        for f, gf in zip(b["fields"], g["fields"]):
            assert f.tobytes() == gf.tobytes(), b["name"]


def test_the_fixture_holds_contraction_witnesses(golden):
    """values whose X differs when s(y) - R is rounded once (a fused multiply-add) instead of twice"""
    b = next(g for g in golden if g["name"] == "witness_f8")
    R, E, st, x = gc.model_of(b)[0]
    assert (float(R), E, st) == (250000.0, 0, 0)
    differ = [j for j, y in enumerate(b["fields"][0]) if gc.one_rounding_x(y, 3, R, E) != int(x[j])]
    assert len(differ) >= 6 and set(range(10, 16)) <= set(differ)


def test_the_fixture_holds_ties_and_a_rounded_down_r(golden):
    for b in (g for g in golden if g["name"].startswith("shapes_")):
        model = gc.model_of(b)
        R, E, st, x = model[6]                                  # ties: t = k + 0.5 exactly, X = k + 1 for even and odd k
        assert (float(R), E) == (0.0, -2)
        t = b["fields"][6].astype(np.float64) * 4.0
        k = np.floor(t)
        half = t - k == 0.5
        assert half[:4].all() and np.array_equal(x[half], (k[half] + 1).astype(np.uint32))
        assert {int(v) % 2 for v in k[:4]} == {0, 1}
        R, E, st, x = model[5]                                  # r_down: R below the minimum, the smallest X above 0
        assert float(R) < float(gc.scale(b["fields"][5].min(), b["D"][5])) and int(x.min()) > 0
        assert model[3][2] == gc.CONSTANT and model[4][2] == gc.CONSTANT and not model[3][3].any()
        z = b["fields"][2]                                      # zeros: both signs present, the minimum is a zero
        assert np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all() and z.min() == 0
        assert float(model[2][0]) == 0.0 and not np.signbit(model[2][0])
        f = b["fields"][0]                                      # ends: the maximum first, the minimum last
        assert f.argmax() == 0 and f.argmin() == f.size - 1


def test_given_parameters_clamp(golden):
    b = next(g for g in golden if g["name"] == "given_f4")
    st = [m[2] for m in gc.model_of(b)]
    assert st == [0, gc.CLAMPED, gc.CLAMPED]


@pytest.mark.skipif(not have_ref(), reason="the compiled reference is not built here")
def test_the_fixture_streams_are_the_references(golden):
    for b in golden:
        nbits, options, bs, rsi = b["tmpl"]
        for x, s in zip(b["X"], b["streams"]):
            if x is not None:
                rc, enc = ref_encode(gc.x_bytes(x, nbits, x.size), nbits, bs, rsi, gc.coder_flags(options, False))
                assert rc == 0 and enc == s, b["name"]


# ---- the cases at the thresholds: grib_cases.edge_batches() and dequantise_cases() ------------------------------------------
EDGES = [b["name"] for b in gc.edge_batches()]
DEQS = [c["name"] for c in gc.dequantise_cases()]


def edge(name):
    return next(b for b in gc.edge_batches() if b["name"] == name)


def deq(name):
    return next(c for c in gc.dequantise_cases() if c["name"] == name)


def bits_of(v):
    v = np.asarray(v)
    return int(v.view(np.uint32 if v.dtype == np.float32 else np.uint64))


def model_against_exact(fields, Ds, nbits, dtype, givens=None):
    """params, quantise and dequantise of the NumPy model against the exact rationals of grib_cases, on every value of
    the fields; returns how many values were compared"""
    M, count = 2 ** nbits - 1, 0
    for i, (f, D) in enumerate(zip(fields, Ds)):
        R, E, st = gc.params(f, D, nbits)
        eR, eE, est = gc.exact_params(f, D, nbits)
        assert st == est, (i, st, est)
        if st & gc.BAD:
            continue
        assert bits_of(R) == bits_of(eR) and E == eE, (i, R, eR, E, eE)
        given = None if givens is None else givens[i]
        if given is not None:
            R, E = np.float32(given[0]), given[1]
        zero = bool(st & gc.CONSTANT) and given is None              # a constant field: X = 0 throughout
        x, clamped = gc.quantise(f, D, nbits, R, E, zero)
        vals, inv = np.unique(f.astype(np.float64), return_inverse=True)
        raw = [0 if zero else gc.exact_x(v, D, R, E) for v in vals]
        want = np.array([min(max(r, 0), M) for r in raw], np.uint64)[inv.ravel()]
        differ = np.flatnonzero(x != want)
        assert differ.size == 0, (i, D, float(R), E, float(f[differ[0]]), int(x[differ[0]]), int(want[differ[0]]))
        assert clamped == any(r < 0 or r > M for r in raw), (i, clamped)
        y = gc.dequantise(x, R, E, D, dtype)
        for xv, j in zip(*np.unique(x, return_index=True)):
            assert bits_of(y[j]) == bits_of(gc.exact_y(xv, R, E, D, dtype)), (i, D, float(R), E, int(xv), y[j])
        count += f.size
    return count


@pytest.mark.parametrize("name", EDGES)
def test_the_model_is_the_exact_rationals_on_the_edge_batches(name):
    b = edge(name)
    assert model_against_exact(b["fields"], b["D"], b["tmpl"][0], b["dtype"], b["given"]) <= sum(f.size for f in b["fields"])


@pytest.mark.parametrize("name", DEQS)
def test_the_model_is_the_exact_rationals_on_the_dequantise_cases(name):
    c = deq(name)
    for (R, E, D), x in zip(c["params"], c["X"]):
        y = gc.dequantise(x, R, E, D, c["dtype"])
        for xv, j in zip(*np.unique(x, return_index=True)):
            assert bits_of(y[j]) == bits_of(gc.exact_y(xv, R, E, D, c["dtype"])), (name, float(R), E, D, int(xv), y[j])


@pytest.mark.parametrize("nbits", gc.NBITS_EDGE)
@pytest.mark.parametrize("D", [0, 3, -2, 22, -22])
@pytest.mark.parametrize("tag", ["f4", "f8"])
def test_the_model_is_the_exact_rationals_on_random_fields(tag, D, nbits):
    """2 000 seeded values, 20 fields of 100: centres of either sign over twelve decades (in units of 10^-D), spreads from
    1e-7 of the centre (at which a float32 field is constant or nearly so) to three times it"""
    dtype = np.dtype(np.float32 if tag == "f4" else np.float64)
    rng = np.random.default_rng([dtype.itemsize, D + 22, nbits])
    fields = []
    for k in range(20):
        centre = float(rng.choice([-1.0, 1.0])) * 10.0 ** rng.uniform(-6, 6)
        s = centre + abs(centre) * 10.0 ** rng.uniform(-7, 0.5) * rng.uniform(-1, 1, 100)
        fields.append((s * 10.0 ** -D).astype(dtype))
    assert model_against_exact(fields, [D] * 20, nbits, dtype) == 2000


def test_the_exact_rationals_round_to_float32_as_the_hardware_does():
    """_rn_f32 (arithmetic on rationals) against the cast of the machine the tests run on, over normals, subnormals, ties
    and the overflow threshold; exact_R against its definition on both sides of a float32"""
    rng = np.random.default_rng(32)
    v = np.concatenate([rng.normal(0, 1, 500) * 10.0 ** rng.integers(-50, 40, 500),
                        [gc.FLT_MAX + 2.0 ** 103, gc.FLT_MAX + 2.0 ** 102, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 2.0 ** -150, 3 * 2.0 ** -150,
                         2.0 ** -126 - 2.0 ** -150, -2.0 ** -151, -0.0, 1e300]])
    with np.errstate(over="ignore", under="ignore"):
        want = v.astype(np.float32)
    assert [bits_of(gc._rn_f32(float(x))) for x in v] == [bits_of(w) for w in want]
    for f in (np.float32(0.1), np.float32(-0.1), np.float32(2.0 ** -149), np.float32(-gc.FLT_MAX)):
        up, down = float(np.nextafter(np.float64(f), np.inf)), float(np.nextafter(np.float64(f), -np.inf))
        assert bits_of(gc.exact_R(float(f))) == bits_of(f) and bits_of(gc.exact_R(up)) == bits_of(f)
        if float(f) > -gc.FLT_MAX:
            assert bits_of(gc.exact_R(down)) == bits_of(np.nextafter(f, np.float32(-np.inf)))


@pytest.mark.parametrize("name", EDGES)
def test_pack_of_the_edge_batches_is_the_models(emul, name):
    check_pack(emul, edge(name))


@pytest.mark.parametrize("name", EDGES)
def test_unpack_of_the_edge_batches_is_the_models(emul, name):
    b = edge(name)
    check_unpack(emul, b, gc.model_of(b))


@pytest.mark.parametrize("name", DEQS)
def test_unpack_of_the_dequantise_cases_is_the_models(emul, name):
    b = gc.deq_as_batch(deq(name))
    check_unpack(emul, b, b["model"])


def test_the_edge_batches_hold_what_they_are_for():
    """every field of every family sits where its generator says: E, status, the bits of R, X at the ends or throughout,
    which values are ties, where the extremes lie.  A generator that moved a case off its threshold fails here."""
    families = set()
    for b in gc.edge_batches():
        families.add((b["family"], "f4" if b["elem"] == 4 else "f8"))
        M = 2 ** b["tmpl"][0] - 1
        for i, (exp, f, D, (R, E, st, x)) in enumerate(zip(b["expect"], b["fields"], b["D"], gc.model_of(b))):
            at = (b["name"], i)
            assert set(exp) <= {"E", "status", "rbits", "x", "xmin", "xmax", "xmax_over", "r_below_min", "ties", "argmin", "argmax"}, at
            assert st == exp["status"], at
            if st & gc.BAD:
                assert x is None and set(exp) == {"status"}, at
                continue
            if "E" in exp:
                assert E == exp["E"], at
            if "rbits" in exp:
                assert bits_of(R) == exp["rbits"], at
            if "x" in exp:
                assert [int(v) for v in x] == exp["x"], at
            if "xmin" in exp:
                assert int(x.min()) == exp["xmin"], at
            if "xmax" in exp:
                assert int(x.max()) == exp["xmax"], at
            if "xmax_over" in exp:
                assert int(x.max()) > exp["xmax_over"] and int(x.max()) <= M, at
            if "r_below_min" in exp:
                assert float(R) < float(gc.scale(f.min(), D)), at
            if "ties" in exp:           # t = k + 0.5 exactly at these, one step below it behind each
                t = f.astype(np.float64) * 4.0
                for j in exp["ties"]:
                    assert t[j] - np.floor(t[j]) == 0.5 and t[j + 1] < t[j] and np.floor(t[j + 1]) == np.floor(t[j]), at
                    assert int(x[j]) == int(np.floor(t[j])) + 1, at
            if "argmin" in exp:
                assert int(f.argmin()) == exp["argmin"] and int(f.argmax()) == exp["argmax"], at
                assert np.count_nonzero(f == f.min()) == 1 and np.count_nonzero(f == f.max()) == 1, at
    # every family is built for both element types, or the list says why not
    said = {(fam, tag) for fam, tag, why in gc.NOT_BUILT if why}
    for fam in {fam for fam, tag in families}:
        for tag in ("f4", "f8"):
            assert (fam, tag) in families or (fam, tag) in said, (fam, tag)
    # the float64 family of E at M: all 96 cases
    assert sum(len(b["fields"]) for b in gc.edge_batches() if b["family"] == "e_at_m" and b["elem"] == 8) == 96
    # positions: every field twice, once on a multiple of 16 bytes and once one element behind one
    for b in (b for b in gc.edge_batches() if b["family"] == "positions"):
        offs, extent = gc.edge_placement(b)
        P, n = gc.position_list(b["elem"])
        assert len(b["fields"]) == 20 and all(f.size == n for f in b["fields"])
        assert [o % 16 for o in offs] == [0, b["elem"]] * 10
        assert sorted({e["argmin"] for e in b["expect"]}) == P == sorted({e["argmax"] for e in b["expect"]})
    # the subnormal float32 values: a conversion that flushed them to zero would give another R (and so other X)
    b = edge("subnormal_f4")
    flushed = [np.zeros_like(f) for f in b["fields"]]
    assert bits_of(gc.params(flushed[0], 22, 16)[0]) != bits_of(gc.model_of(b)[0][0])


def test_the_dequantise_cases_hold_what_they_are_for():
    """the Y the model gives at the spots each case names: the ties to even, Inf, the subnormals, the exact +0.0; and the
    run lengths on either side of a lane's group"""
    for c in gc.dequantise_cases():
        per = 16 // gc.container(c["tmpl"][0])
        sizes = {x.size for x in c["X"]}
        assert sizes == {1, per - 1, per, per + 1, 64 * per + 1}, c["name"]
        for (R, E, D), x, spots in zip(c["params"], c["X"], c["expect"]):
            y = gc.dequantise(x, R, E, D, c["dtype"])
            for xv, bits in spots.items():
                for j in np.flatnonzero(x == xv)[:1]:
                    assert bits_of(y[j]) == bits, (c["name"], float(R), E, D, xv, hex(bits_of(y[j])))
    sub = deq("deq_subnormal_f4")
    y = np.concatenate([gc.dequantise(x, R, E, D, np.float32) for (R, E, D), x in zip(sub["params"], sub["X"])])
    assert np.count_nonzero((y != 0) & (np.abs(y) < 2.0 ** -126)) > 100
