"""aec_gpu_encode_chunks_plan (include/aec_gpu.h; host arithmetic, no device): waves, RSI table entries, output bound and
refusals against a restatement in Python.  The restatement follows the header's comment for out_bound and rsi_entries, and
aec_enc.hip's make_geom for the segments a wave walks: as many as 8 while the batch has at least 2048 segments per wave of
a workgroup to hand out, halved until it has."""
import numpy as np
import pytest

import helpers
from helpers import AEC_DATA_3BYTE, AEC_DATA_MSB, AEC_DATA_PREPROCESS as PP, AEC_DATA_SIGNED, AEC_NOT_ENFORCE, AEC_RESTRICTED

from libaec_amd import gpu

PARAMS = [
    (8, 8, 128, PP),
    (16, 16, 64, PP),
    (16, 16, 128, 0),
    (32, 32, 100, PP | AEC_DATA_MSB | AEC_DATA_SIGNED),
    (24, 64, 17, PP | AEC_DATA_3BYTE),
    (12, 24, 5, PP | AEC_NOT_ENFORCE),
    (8, 8, 1, PP),
    (32, 64, 4096, PP),
]


def geometry(bps, bs, rsi, flags):
    nbytes = helpers.bytes_per_sample(bps, flags)
    return nbytes, helpers.id_len_of(bps, flags), (rsi + 63) // 64


def counts(size, bps, bs, rsi, flags):
    nbytes, _, spr = geometry(bps, bs, rsi, flags)
    samples = size // nbytes
    blocks = (samples + bs - 1) // bs
    return blocks, (blocks // rsi) * spr + (blocks % rsi + 63) // 64, (blocks + rsi - 1) // rsi


def segs_per_wave(total_segs, bps, bs, rsi, flags):
    """aec_enc.hip make_geom(c, with_obuf=True)"""
    nbytes, id_len, _ = geometry(bps, bs, rsi, flags)
    templated = bs in (8, 16, 32, 64)
    stride = bs // 2 + 4 if templated and nbytes <= 2 else bs + 4
    maxlen = id_len + bs * bps + 2 + bps
    obuf_words = ((64 * maxlen + 62) // 32 + 4) & ~3
    per_wave = (64 * stride + obuf_words) * 4
    wpb = min(max(65536 // per_wave, 1), 4)
    spw = 8
    while spw > 1 and total_segs < spw * wpb * 2048:
        spw >>= 1
    return spw


def restated(sizes, bps, bs, rsi, flags):
    _, id_len, _ = geometry(bps, bs, rsi, flags)
    per = [counts(int(s), bps, bs, rsi, flags) for s in sizes]
    spw = segs_per_wave(sum(p[1] for p in per), bps, bs, rsi, flags)
    bound = sum(max(1, (p[0] * (id_len + bs * bps + 2) + 7) // 8) for p in per)
    return {"out_bound": (bound + 15) // 16 * 16 + 16, "rsi_entries": sum(p[2] + 1 for p in per),
            "waves": sum((p[1] + spw - 1) // spw for p in per)}


def edge_sizes(bps, bs, rsi, flags):
    nbytes, _, spr = geometry(bps, bs, rsi, flags)
    blk, rsi_b = bs * nbytes, bs * nbytes * rsi

    def of_segs(k):                     # a chunk of exactly k segments
        full, rem = divmod(k, spr)
        return full * rsi_b + rem * 64 * blk

    return [0, nbytes, (bs - 1) * nbytes, blk, rsi_b - blk, rsi_b, rsi_b + nbytes, of_segs(2048), of_segs(2049), of_segs(4100),
            blk * 64, blk * 65, nbytes - 1 if nbytes > 1 else 0, rsi_b + nbytes + (nbytes - 1)]


def check(sizes, prm):
    got = gpu.encode_chunks_plan(*prm, sizes)
    assert got is not None, (prm, list(sizes))
    want = restated(sizes, *prm)
    for key, val in want.items():
        assert got[key] == val, (key, prm, list(sizes))
    assert got["workspace_bytes"] > 0
    return got


@pytest.mark.parametrize("prm", PARAMS, ids=lambda p: "-".join(str(x) for x in p))
def test_every_edge_size_alone_and_together(prm):
    sizes = edge_sizes(*prm)
    for s in sizes:
        check([s], prm)
    check(sizes, prm)
    check(sizes[::-1], prm)
    rng = np.random.default_rng(prm[0] * 7 + prm[2])
    for _ in range(6):
        check(rng.choice(sizes, size=int(rng.integers(2, 40))).tolist(), prm)


def test_the_chunks_of_2049_and_4100_segments_count_for_what_they_are():
    prm = (8, 8, 128, PP)
    for segs in (2048, 2049, 4100):
        got = check([segs * 64 * 8, 24], prm)
        assert got["waves"] == segs + 1 and got["rsi_entries"] == (segs + 1) // 2 + 1 + 2      # (two segments per RSI)


def test_every_segs_per_wave_of_config_5():
    """16384 / 32768 / 65536 segments of config 5 (512 bytes each: 8 / 16 / 32 MiB) are where a wave begins to walk 2 / 4 / 8
    segments; the segments of all chunks together count, and a chunk's last wave is its own"""
    prm = (8, 8, 128, PP)
    for thresh, spw in ((16384, 2), (32768, 4), (65536, 8)):
        for total, per_wave in ((thresh, spw), (thresh - 1, spw // 2)):
            segs = [total - 1005, 1000, 5]
            got = check([k * 512 for k in segs], prm)
            assert got["waves"] == sum(-(-k // per_wave) for k in segs)


def test_no_chunks_is_a_plan_of_nothing():
    got = gpu.encode_chunks_plan(8, 8, 128, PP, [])
    assert got is not None and got["waves"] == 0 and got["rsi_entries"] == 0 and got["out_bound"] == 16


@pytest.mark.parametrize("prm", [
    (0, 8, 128, PP), (33, 8, 128, PP), (8, 10, 128, PP), (8, 7, 128, PP | AEC_NOT_ENFORCE), (8, 8, 0, PP), (8, 8, 4097, PP),
    (8, 66, 16, PP | AEC_NOT_ENFORCE), (1, 8, 16, AEC_DATA_SIGNED), (6, 8, 16, AEC_RESTRICTED),
])
def test_what_check_params_refuses_the_plan_refuses(prm):
    from libaec_amd.gpu import Params, _lib
    import ctypes as C
    assert _lib().aec_gpu_check_params(C.byref(Params(*prm)), 1) != 0
    assert gpu.encode_chunks_plan(*prm, [1000, 2000]) is None
    assert gpu.encode_chunks_plan(*prm, []) is None
