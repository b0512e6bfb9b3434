"""The short-block and narrow-sample corner of what aec_decode_init accepts -- what the SZIP filter sends (sz_abi.cpp: any
even block size from 2 to 32 with AEC_NOT_ENFORCE, pixels from 1 bit up) and what AEC_RESTRICTED adds (block headers of
one and two bits) -- as the cases tests/test_narrow_emul.py runs through the CPU emulations and tests/test_gpu_narrow.py on
the device: the parameter sets in four classes, the data, the streams built from them and the oracle's answer.  Not a test
module.

Coded data sets are a few bits long here, where the index pass's tables and windows were sized on 8-, 16- and 32-bit
samples in blocks of 8 to 64 (a candidate per 12 bits in the window tables, hop records of 15 and 18 bits in the every-bit
scheme, rules on the header length in the phase-locked chains).

  CASES      ~30 parameter sets with a data kind each; `family(case)` is the stream the decode families take
  DISPATCH   per class, the streams of 0.25 to 2.2 MiB the shipped index pass sends to the phase-locked chains, the
             window tables and the trunk (tests/golden/narrow_chain.json pins the chains; tests/golden/make_golden_narrow.py)
  FORCED     the shapes of tests/cross_scheme.py --narrow, every legal scheme forced on each
  SZ_SHAPES  two SZIP chunks of 1 MiB against the reference shim's bytes (tests/golden/narrow_sz.json)
"""
import hashlib
import json
import os
import sys
import zlib
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from helpers import (AEC_DATA_3BYTE, AEC_DATA_MSB, AEC_DATA_PREPROCESS, AEC_DATA_SIGNED, AEC_NOT_ENFORCE, AEC_OK,  # noqa: E402
                     AEC_RESTRICTED, OPT_SE, OPT_SPLIT, OPT_UNCOMP, OPT_ZERO, bytes_per_sample, derive, id_len_of,
                     oracle_decode, oracle_encode, pack_samples, random_walk_samples)

PP, MSB, SGN, B3, R, NE = (AEC_DATA_PREPROCESS, AEC_DATA_MSB, AEC_DATA_SIGNED, AEC_DATA_3BYTE, AEC_RESTRICTED,
                           AEC_NOT_ENFORCE)
CLASSES = ("generic", "narrow", "restricted", "odd")
KINDS = ("walk", "noise", "specks", "bits01")
RSIS = (1, 5, 16, 44, 45, 64, 65, 128, 300, 4096)
BASE = 1 << 18                  # samples generated per stream at the most; longer streams are tiles of them

Case = namedtuple("Case", "cls bps bs rsi flags kind short")

# short: the mean coded data set of the case's streams is below 8 bits (the window tables are sized for 12 and more)
CASES = [
    # generic blocks: bs in {2, 4, 6, 10, 24, 62} with AEC_NOT_ENFORCE, bps 1, 5, 8, 12, 16, 31
    Case("generic", 1, 2, 64, PP | NE, "walk", True),
    Case("generic", 1, 2, 4096, PP | NE, "bits01", True),
    Case("generic", 5, 2, 128, PP | NE, "walk", True),
    Case("generic", 8, 4, 5, PP | NE | MSB, "specks", True),
    Case("generic", 12, 62, 5, PP | NE, "walk", False),
    Case("generic", 16, 6, 300, PP | NE | MSB, "walk", False),
    Case("generic", 31, 6, 65, PP | NE, "noise", False),
    Case("generic", 8, 10, 45, NE, "noise", False),                  # without the preprocessor
    Case("generic", 5, 24, 16, PP | NE, "walk", False),
    # narrow samples with three header bits: bs 8 and 16 as well as generic
    Case("narrow", 1, 8, 128, PP, "bits01", False),
    Case("narrow", 2, 16, 16, PP, "walk", False),
    Case("narrow", 3, 8, 4096, PP, "noise", False),
    Case("narrow", 5, 16, 65, PP | MSB, "walk", False),
    Case("narrow", 7, 8, 1, PP, "walk", False),
    Case("narrow", 2, 4, 44, PP | NE, "specks", True),
    Case("narrow", 3, 10, 300, PP | NE, "walk", False),
    Case("narrow", 7, 16, 64, 0, "noise", False),                    # without the preprocessor
    Case("narrow", 1, 6, 5, PP | NE, "walk", True),
    # restricted sets: one header bit (bps 1, 2), two (bps 3, 4), bs 2, 4, 16, 64
    Case("restricted", 1, 16, 64, PP | R, "bits01", False),
    Case("restricted", 2, 2, 16, PP | NE | R, "walk", True),
    Case("restricted", 2, 4, 128, PP | NE | R, "walk", True),
    Case("restricted", 3, 64, 5, PP | R, "walk", False),
    Case("restricted", 4, 64, 4096, PP | R, "specks", False),
    Case("restricted", 4, 16, 45, PP | R, "walk", False),
    Case("restricted", 1, 2, 300, PP | NE | R, "specks", True),
    Case("restricted", 3, 4, 65, PP | NE | R, "walk", True),
    Case("restricted", 4, 2, 1, R | NE, "noise", False),             # without the preprocessor, rsi 1
    # odd containers: 3-byte samples, 31 bits, both byte orders, signed where samples come back as they went in
    Case("odd", 12, 16, 64, PP | B3 | MSB, "walk", False),
    Case("odd", 20, 8, 16, PP | B3, "walk", False),
    Case("odd", 24, 24, 300, PP | NE | B3, "walk", False),
    Case("odd", 24, 32, 5, PP | B3 | MSB | SGN, "noise", False),
    Case("odd", 31, 16, 128, PP | MSB, "walk", False),
    Case("odd", 20, 64, 1, PP | B3 | MSB, "noise", False),
    Case("odd", 31, 8, 4096, PP, "specks", False),
    Case("odd", 31, 10, 44, NE | MSB, "noise", False),               # without the preprocessor: split options up to kmax
]


def case_id(c):
    return f"{c.cls}-n{c.bps}-j{c.bs}-r{c.rsi}-f{c.flags}-{c.kind}"


def prm(c):
    return (c.bps, c.bs, c.rsi, c.flags)


def of_class(cls, cases=None):
    return [c for c in (CASES if cases is None else cases) if c.cls == cls]


def value_range(bps, flags):
    if flags & SGN:
        return -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    return 0, (1 << bps) - 1


def _stretches(rng, v, bs, lo, hi):
    """constant stretches of whole blocks laid over v: zero runs of 1 to 4 blocks, of 6 and more, and one that reaches
    the end of its segment whatever the RSI (70 blocks and more: a rest-of-segment code)"""
    n = v.size
    for blocks in (1, 2, 3, 4, 6, 9, 70, 140):
        for _ in range(3):
            ln = blocks * bs + 1
            if ln * 4 > n:
                continue
            s = int(rng.integers(1, n - ln)) // bs * bs
            v[s:s + ln] = v[s - 1] if s else v[0]
    return v


def make_values(rng, kind, n, bps, flags, bs=8):
    lo, hi = value_range(bps, flags)
    if kind == "walk":          # scale 0.3 to 1 with constant stretches: zero runs, second extension, k = 0
        v = random_walk_samples(rng, n, bps, flags, scale=float(rng.choice([0.3, 0.5, 1.0])), zero_frac=0.1, jump_frac=0.003)
        # (a stretch of small steps of both signs -- split with k = 0 and 1 -- and stretches of noise of every amplitude)
        q = n // 8
        if q > 8 * bs:
            v[q:2 * q] = np.clip(v[q] + np.cumsum(rng.integers(-1, 2, size=q)), lo, hi)
            a, w, m = n - q, min(4 * bs, max(bs, q // (bps + 1) // bs * bs)), (lo + hi) // 2
            for e in range(bps + 1):
                if a + w > n:
                    break
                half = (1 << e) // 2
                v[a:a + w] = rng.integers(max(lo, m - half), min(hi, m + half) + 1, size=w, dtype=np.int64)
                a += w
        return _stretches(rng, v, bs, lo, hi)
    if kind == "noise":         # uncompressed blocks, and stretches of every amplitude below (every split option)
        v = rng.integers(lo, hi + 1, size=n, dtype=np.int64)
        w = max(2 * bs, min(16 * bs, n // (4 * (bps + 1)) // bs * bs))
        a = n // 3 // bs * bs
        for e in range(bps, -1, -1):
            if a + w > n:
                break
            base = int(rng.integers(lo, hi + 1 - ((1 << e) - 1)))
            v[a:a + w] = base + rng.integers(0, 1 << e, size=w, dtype=np.int64)
            a += w
        return _stretches(rng, v, bs, lo, hi) if n >= 2048 * bs else v
    if kind == "specks":        # a constant with specks: runs of zero blocks, rest-of-segment codes
        v = np.full(n, lo + (hi - lo) // 3, np.int64)
        m = rng.random(n) < 0.004
        v[m] = rng.integers(lo, hi + 1, size=int(m.sum()), dtype=np.int64)
        return v
    if kind == "bits01":        # values 0 and 1 only: second extension, k = 0, and stretches of either value
        v = rng.integers(0, 2, size=n, dtype=np.int64)
        return _stretches(rng, v, bs, lo, hi)
    raise ValueError(kind)


_data_cache = {}


def case_data(c, n, salt=0):
    """n samples of the case's kind as bytes: a base of at most BASE samples, tiled"""
    key = (c, min(n, BASE), salt)
    if key not in _data_cache:
        if len(_data_cache) > 64:
            _data_cache.clear()
        rng = np.random.default_rng(zlib.crc32(repr((tuple(c), salt)).encode()))
        _data_cache[key] = pack_samples(make_values(rng, c.kind, min(n, BASE), c.bps, c.flags, c.bs), c.bps, c.flags)
    base = _data_cache[key]
    nb = bytes_per_sample(c.bps, c.flags)
    return np.ascontiguousarray(np.tile(base, -(-n * nb // base.size))[: n * nb])


Coded = namedtuple("Coded", "data stream offs bits trace decoded nblk")
_coded_cache = {}


def coded(c, n, salt=0, want_trace=True):
    """the oracle's answer for n samples of the case: stream, RSI start bits, total bits, per-block trace, decoded bytes"""
    key = (c, n, salt)
    if key not in _coded_cache:
        if len(_coded_cache) > 48:
            _coded_cache.clear()
        data = case_data(c, n, salt)
        rc, stream, trace, offs, bits = oracle_encode(data, *prm(c), want_trace=want_trace)
        assert rc == AEC_OK and len(stream) == max(1, (bits + 7) // 8)
        nblk = -(-n // c.bs)
        cap = nblk * c.bs * bytes_per_sample(c.bps, c.flags)
        rc, dec, _ = oracle_decode(stream, *prm(c), cap)
        assert rc == AEC_OK and len(dec) == cap
        _coded_cache[key] = Coded(data, stream, offs.astype(np.uint64), int(bits), trace, dec, nblk)
    return _coded_cache[key]


def wave_kernel(c, n_rsi=3):
    """does the table decode of n_rsi RSIs of this shape take the wave kernel (aec_dec.hip: dec_wave_wanted)"""
    return c.bs in (8, 16, 32, 64) and c.rsi >= 16


def family_samples(c):
    """70 RSIs and a short last one -- one wavefront of lanes and six lanes of a second -- where a lane takes an RSI; two
    RSIs and a short last one where a wavefront does; half a block more at the end"""
    whole = 2 if wave_kernel(c) else 70
    last = 65 if c.rsi > 65 else max(1, c.rsi // 3)
    return (whole * c.rsi + last) * c.bs - (c.bs // 2 if last > 1 else 0)


def family(c):
    return coded(c, family_samples(c))


# ---- what a trace holds -------------------------------------------------------------------------------------

FEATURES = ("zero run of 1-4 blocks", "zero run of 6 blocks or more", "rest-of-segment run", "second extension",
            "split k = 0", "split k = kmax", "uncompressed")


def kmax_of(c):
    rc, d = derive(*prm(c))
    assert rc == 0
    return d.kmax


def features(c, trace):
    """which of FEATURES the blocks of a trace show.  A run of zero blocks is the block that carries its code and the
    blocks it swallowed; its fundamental sequence is 5 bits long for "the rest of the segment" and for nothing else
    (1 to 4 blocks: 1 to 4 bits; 5 blocks and more: 6 and more)."""
    opt, k, bits = trace["option"], trace["k"], trace["bits"].astype(np.int64)
    idl, kmax = id_len_of(c.bps, c.flags), kmax_of(c)
    got = set()
    zero = np.flatnonzero(opt == OPT_ZERO)
    if zero.size:
        ref = np.where((zero % c.rsi == 0) & bool(c.flags & PP), c.bps, 0)
        fs = bits[zero] - idl - 1 - ref
        if np.any((fs >= 1) & (fs <= 4)):
            got.add(FEATURES[0])
        if np.any(fs >= 7):
            got.add(FEATURES[1])
        if np.any(fs == 5):
            got.add(FEATURES[2])
    if np.any(opt == OPT_SE):
        got.add(FEATURES[3])
    split = opt == OPT_SPLIT
    if np.any(split & (k == 0)):
        got.add(FEATURES[4])
    if kmax > 0 and np.any(split & (k == kmax)):
        got.add(FEATURES[5])
    if np.any(opt == OPT_UNCOMP):
        got.add(FEATURES[6])
    return got


def mean_cds_bits(trace):
    return float(trace["bits"].sum()) / max(1, len(trace))


# ---- the streams of the index pass ---------------------------------------------------------------------------

SERIAL, LOCKED, TABLES, TRUNK, EVERY_BIT, REGIONS = range(6)

# (case, samples, first scheme): per class, the smallest stream of the ladder 256 KiB, 640 KiB, 2.2 MiB (the every-bit
# scheme's own 2^24 bits are behind it there) whose chain begins with the phase-locked chains, the window tables, the
# trunk.  No class needs more than 8 MiB of stream for any of the three.
DISPATCH = [
    (Case("generic", 1, 2, 64, PP | NE, "walk", True), 3_887_402, LOCKED),
    (Case("generic", 5, 2, 128, PP | NE, "walk", True), 864_852, TABLES),
    (Case("generic", 16, 6, 4096, PP | NE | MSB, "walk", False), 6_692_862, TRUNK),
    (Case("narrow", 7, 8, 1, PP, "walk", False), 5_604_656, LOCKED),
    (Case("narrow", 1, 8, 128, PP, "bits01", False), 1_570_128, TABLES),
    (Case("narrow", 3, 8, 4096, PP, "noise", False), 5_483_176, TRUNK),
    (Case("restricted", 2, 2, 16, PP | NE | R, "noise", True), 7_518_570, LOCKED),
    (Case("restricted", 2, 4, 128, PP | NE | R, "walk", True), 1_761_448, TABLES),
    (Case("restricted", 4, 64, 4096, PP | R, "noise", False), 5_068_096, TRUNK),
    (Case("odd", 24, 32, 5, PP | B3 | MSB | SGN, "noise", False), 826_752, LOCKED),
    (Case("odd", 31, 16, 128, PP | MSB, "walk", False), 547_488, TABLES),
    (Case("odd", 31, 8, 4096, 0, "specks", False), 567_976, TRUNK),
]

# (case, input bytes): the shapes of tests/cross_scheme.py --narrow, whole blocks each
FORCED = [
    (Case("generic", 1, 2, 64, PP | NE, "walk", True), 2 << 20),
    (Case("generic", 16, 6, 300, PP | NE | MSB, "walk", False), 1 << 20),
    (Case("generic", 5, 2, 128, PP | NE, "walk", True), 600 << 10),
    (Case("generic", 12, 62, 5, PP | NE, "walk", False), 600 << 10),
    (Case("narrow", 1, 8, 128, PP, "bits01", False), 1 << 20),
    (Case("narrow", 3, 8, 4096, PP, "noise", False), 3 << 20),
    (Case("narrow", 2, 4, 44, PP | NE, "specks", True), 100 << 10),
    (Case("narrow", 5, 16, 65, PP | MSB, "walk", False), 1 << 20),
    (Case("narrow", 7, 8, 1, PP, "walk", False), 3 << 20),
    (Case("restricted", 2, 2, 16, PP | NE | R, "walk", True), 600 << 10),
    (Case("restricted", 2, 4, 128, PP | NE | R, "walk", True), 1 << 20),
    (Case("restricted", 4, 64, 4096, PP | R, "noise", False), 3 << 20),
    (Case("odd", 24, 24, 300, PP | NE | B3, "walk", False), 3 << 20),
    (Case("odd", 31, 16, 128, PP | MSB, "walk", False), 600 << 10),
    (Case("odd", 20, 8, 16, PP | B3, "walk", False), 100 << 10),
]


def forced_samples(c, nbytes):
    """whole RSIs: a run of zero blocks that closes a short last RSI reads as one to the end of its segment, and the script
    asserts the exact count of RSIs (the short last RSI is the decode families' and the shipped dispatch's)"""
    return nbytes // bytes_per_sample(c.bps, c.flags) // (c.bs * c.rsi) * (c.bs * c.rsi)


def rsi_bits_hint(k):
    """the mean coded RSI, as tests/cross_scheme.py hands it to aec_gpu_index_scheme"""
    return k.bits // max(1, len(k.offs))


def legal_schemes(c, k):
    """the schemes aec_gpu_index_scheme names for stream k of case c as the tuning build's switches take them away one after
    the other -- the walk of tests/cross_scheme.py, host arithmetic; AEC_AMD_LIB must name the tuning build"""
    import os
    from cross_scheme import KNOBS, OFF, ORDER
    from libaec_amd import gpu
    assert "tuning" in os.environ.get("AEC_AMD_LIB", ""), "the switches exist in the tuning build only"
    taken, disabled = [], {}
    for s in ORDER:
        for knob in KNOBS:
            os.environ.pop(knob, None)
        os.environ.update(disabled)
        os.environ["AEC_IDX_REGIONS_MIN"] = "0"
        scheme = gpu.index_scheme(*prm(c), len(k.stream), rsi_bits_hint(k), 0)
        if s in OFF:
            disabled = {**disabled, **OFF[s]}
        if scheme == s and scheme not in taken:
            taken.append(scheme)
    for knob in KNOBS:
        os.environ.pop(knob, None)
    return taken


def forced_table():
    """{case id: in_bytes, rsi_bits, schemes} of FORCED, under the tuning build"""
    out = {}
    for c, nbytes in FORCED:
        k = coded(c, forced_samples(c, nbytes))
        out[case_id(c)] = {"in_bytes": len(k.stream), "rsi_bits": rsi_bits_hint(k), "schemes": legal_schemes(c, k)}
    return out


def dispatch_table():
    """the rows of DISPATCH with what aec_gpu_index_plan says of the shipped library's pass over each stream"""
    from libaec_amd import gpu
    rows = []
    for c, n, first in DISPATCH:
        k = coded(c, n)
        ids = gpu.index_plan(*prm(c), len(k.stream), rsi_bits_hint(k))[0]
        rows.append({"case": case_id(c), "class": c.cls, "samples": n, "in_bytes": len(k.stream), "rsi_bits": rsi_bits_hint(k),
                     "mean_cds_bits": round(mean_cds_bits(k.trace), 2), "first_scheme": first, "chain": ids})
    return rows


GOLDEN_CHAINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "narrow_chain.json")


def golden_chains():
    with open(GOLDEN_CHAINS) as f:
        return json.load(f)


if __name__ == "__main__":      # `python tests/narrow_cases.py forced`: forced_table() as JSON (a child of the CPU test)
    import sys
    assert sys.argv[1:] == ["forced"]
    print(json.dumps(forced_table()))


# ---- SZIP ----------------------------------------------------------------------------------------------------

GOLDEN_SZ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "narrow_sz.json")
SZ_NN, SZ_MSB, SZ_RAW = 32, 16, 128         # (include/szlib.h)
# (name, (options, bits per pixel, pixels per block, pixels per scan line), data kind): one chunk of 1 MiB each
SZ_SHAPES = [("1-bit pixels, 2 per block, lines of 128", (SZ_NN | SZ_RAW, 1, 2, 128), "walk"),
             ("5-bit pixels, 10 per block, lines of 1000", (SZ_NN | SZ_MSB | SZ_RAW, 5, 10, 1000), "walk")]


def sz_chunks():
    """(name, parameters, 1 MiB of pixels) per SZIP shape; the last scan line of the second is incomplete"""
    for name, p, kind in SZ_SHAPES:
        c = Case("sz", p[1], p[2], -(-p[3] // p[2]), PP | NE, kind, p[1] * p[2] < 8)
        yield name, p, case_data(c, 1 << 20)


def sz_golden():
    """[(name, parameters, input, length and SHA-256 of the reference shim's stream)] of tests/golden/narrow_sz.json.
    Two streams of 1 MiB chunks are 420 KB that do not compress: the fixture holds their digests, and the digest of the
    input the stream was made of, which sz_chunks() must give again."""
    with open(GOLDEN_SZ) as f:
        rows = json.load(f)
    out = []
    for row, (name, p, data) in zip(rows, sz_chunks()):
        assert (row["name"], tuple(row["params"])) == (name, p)
        assert hashlib.sha256(data.tobytes()).hexdigest() == row["input_sha256"], f"{name}: the generated input is not the fixture's"
        out.append((name, p, data, row["stream_bytes"], row["stream_sha256"]))
    return out
