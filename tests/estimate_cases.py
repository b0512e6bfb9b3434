"""The cases of the size estimate (include/aec_gpu.h: aec_gpu_estimate_async) that tests/test_estimate_emul.py runs
through the CPU emulation and tests/test_gpu_estimate.py on the device: the parameter sets, the RSI vectors, the lengths
and the data, and the oracle's answer for a candidate.  Not a test module."""
import numpy as np

from helpers import (AEC_DATA_3BYTE, AEC_DATA_MSB, AEC_DATA_PREPROCESS, AEC_DATA_SIGNED, AEC_RESTRICTED,
                     bytes_per_sample, oracle_encode, pack_samples, random_walk_samples)

PP, MSB, SIGNED, B3, RESTRICTED = AEC_DATA_PREPROCESS, AEC_DATA_MSB, AEC_DATA_SIGNED, AEC_DATA_3BYTE, AEC_RESTRICTED

PARAMS = [(8, PP), (16, PP | MSB), (16, PP | SIGNED), (12, PP), (24, PP | B3), (32, PP), (32, PP | SIGNED | MSB), (16, 0),
          (32, 0), (4, PP | RESTRICTED), (2, PP | RESTRICTED), (1, PP)]

RSI_ALL = 17          # p->rsi of every case: what an RSI vector of None stands for
RSI_VECTORS = [[128] * 4, [1] * 4, [3, 5, 7, 2], [65] * 4, [4096] * 4, [16, 8, 4, 2], [0, 16, 0, 0], None]

LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65, 511, 513, 4096 + 17]

KINDS = ["walk", "zero", "const", "noise", "ends", "bits01"]


def param_id(p):
    return f"n{p[0]}f{p[1]}"


def value_range(bps, flags):
    if flags & SIGNED:
        return -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    return 0, (1 << bps) - 1


def make_values(rng, kind, n, bps, flags):
    lo, hi = value_range(bps, flags)
    if kind == "walk":          # mixed entropy with constant stretches (zero blocks behind the predictor)
        return random_walk_samples(rng, n, bps, flags)
    if kind == "zero":
        return np.zeros(n, np.int64)
    if kind == "const":
        return np.full(n, lo + (hi - lo) // 3, np.int64)
    if kind == "noise":         # 32 bits without the predictor: pair sums beyond 2^32, fs(0) beyond 32 bits
        return rng.integers(lo, hi + 1, size=n, dtype=np.int64)
    if kind == "ends":          # both ends of the range: the clipping branch of the predictor
        return rng.choice(np.array([lo, min(lo + 1, hi), max(hi - 1, lo), hi], np.int64), size=n)
    if kind == "bits01":        # favours the second extension
        return rng.integers(0, 2, size=n, dtype=np.int64) + (0 if hi >= 1 else lo)
    raise ValueError(kind)


def make_data(rng, kind, n, bps, flags):
    return pack_samples(make_values(rng, kind, n, bps, flags), bps, flags)


def rsi_of(vec, i):
    return RSI_ALL if vec is None else vec[i]


def crafted_zero_runs(rng, bps, flags, vec):
    """Zero runs of 4, 5, 64 and 65 blocks of 8 samples at 0, 8 and 24 samples behind an RSI start of the first size asked
    for, in data that has no other zero block: the same bytes give each size its own runs, rest-of-segment codes and run
    starts on reference slots."""
    lo, hi = value_range(bps, flags)
    first = next(i for i in range(4) if rsi_of(vec, i))
    period = rsi_of(vec, first) * (8 << first)
    stride = period * -(-700 // period)
    places = [(blocks * 8, off) for blocks in (4, 5, 64, 65) for off in (0, 8, 24)]
    n = stride * (len(places) + 1) + 17
    if flags & PP:              # a step of 2 to 4 up, then down, at every sample: no residual is zero ...
        wide = hi - lo
        a = 3 if wide >= 5 else (2 if wide >= 3 else 1)
        r = rng.integers(0, 2, size=n) if wide >= 3 else np.zeros(n, np.int64)
        v = lo + max(0, wide // 2 - 2) + (np.arange(n) % 2) * a + r
        assert v.max() <= hi and np.all(np.diff(v) != 0)
    else:                       # ... without the predictor: no sample is zero
        v = rng.integers(1, min(hi, 200) + 1, size=n, dtype=np.int64)
    for j, (length, off) in enumerate(places):
        s = (j + 1) * stride + off
        v[s:s + length] = v[s - 1] if flags & PP else 0
    return pack_samples(v, bps, flags)


_oracle_cache = {}


def oracle_bits(key, data, bps, flags, i, rsi):
    """total bits (and, with trace, the per-block trace) of candidate i; cached per data set `key`"""
    k = (key, bps, flags, i, rsi)
    if k not in _oracle_cache:
        if len(_oracle_cache) > 4096:
            _oracle_cache.clear()
        rc, enc, trace, _, bits = oracle_encode(data, bps, 8 << i, rsi, flags, want_trace=True)
        assert rc == 0
        _oracle_cache[k] = (bits, trace, len(enc))
    return _oracle_cache[k]


def expected(key, data, bps, flags, vec):
    """(total_bits[4], best) as aec_gpu_estimate defines them"""
    totals = []
    for i in range(4):
        r = rsi_of(vec, i)
        totals.append(oracle_bits(key, data, bps, flags, i, r)[0] if r else (1 << 64) - 1)
    asked = [i for i in range(4) if rsi_of(vec, i)]
    best = min(asked, key=lambda i: (totals[i], i))
    return totals, best


def samples_of(data, bps, flags):
    return len(data) // bytes_per_sample(bps, flags)
