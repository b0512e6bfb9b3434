"""aec_gpu_decode_chunks_plan (include/aec_gpu.h; host arithmetic, no device): items, RSI table entries and the packed
output of a batch of chunks that decode to given sizes, against a restatement in Python; the table's entries must be those
aec_gpu_encode_chunks_plan counts for chunks of the same sizes -- the table the encoder writes is the one the decoder takes."""
import ctypes as C

import numpy as np
import pytest

import helpers
from helpers import AEC_DATA_3BYTE, AEC_DATA_MSB, AEC_DATA_PREPROCESS as PP, AEC_DATA_SIGNED, AEC_NOT_ENFORCE, AEC_RESTRICTED

from libaec_amd import gpu

C5 = (8, 8, 128, PP)
PARAM_SETS = [                                               # (those of tests/test_gpu_encode_chunks.py)
    C5,
    (16, 16, 64, PP),
    (16, 16, 128, 0),
    (32, 32, 100, PP | AEC_DATA_MSB | AEC_DATA_SIGNED),
    (24, 64, 17, PP | AEC_DATA_3BYTE),
    (12, 24, 5, PP | AEC_NOT_ENFORCE),
    (16, 8, 1, PP),
]


def counts(size, prm):
    bps, bs, rsi, flags = prm
    nb = helpers.bytes_per_sample(bps, flags)
    blocks = (size // nb + bs - 1) // bs
    return blocks, (blocks + rsi - 1) // rsi, bs * nb


def restated(sizes, prm):
    per = [counts(int(s), prm) for s in sizes]
    return {"items": sum(p[1] for p in per), "rsi_entries": sum(p[1] + 1 for p in per),
            "out_bytes": sum((p[0] * p[2] + 15) // 16 * 16 for p in per)}


def edge_sizes(prm):
    bps, bs, rsi, flags = prm
    nb = helpers.bytes_per_sample(bps, flags)
    blk, rsi_b = bs * nb, bs * nb * rsi
    return [0, nb - 1 if nb > 1 else 0, nb, (bs - 1) * nb, 64 * blk, 65 * blk, rsi_b, rsi_b + nb, 3 * rsi_b + 7 * nb,
            rsi_b + nb + (nb - 1), 5 * rsi_b]


def check(sizes, prm):
    got = gpu.decode_chunks_plan(*prm, sizes)
    assert got is not None, (prm, list(sizes))
    for key, val in restated(sizes, prm).items():
        assert got[key] == val, (key, prm, list(sizes))
    assert got["rsi_entries"] == gpu.encode_chunks_plan(*prm, sizes)["rsi_entries"]
    assert got["workspace_bytes"] >= 4 * got["items"] + 40 * (len(sizes) + 1)
    return got


@pytest.mark.parametrize("prm", PARAM_SETS, ids=lambda p: "-".join(str(x) for x in p))
def test_every_edge_size_alone_and_together(prm):
    sizes = edge_sizes(prm)
    for s in sizes:
        check([s], prm)
    check(sizes, prm)
    check(sizes[::-1], prm)
    rng = np.random.default_rng(prm[0] * 7 + prm[2])
    for _ in range(6):
        check(rng.choice(sizes, size=int(rng.integers(2, 40))).tolist(), prm)


def test_no_chunks_is_a_plan_of_nothing():
    got = gpu.decode_chunks_plan(*C5, [])
    assert got is not None and got["items"] == 0 and got["rsi_entries"] == 0 and got["out_bytes"] == 0


def test_more_items_than_a_launch_addresses_are_refused():
    """2^31 - 1 items at the most (a grid's workgroups): RSIs of 8 bytes, so 16 GiB announced is one item too many"""
    prm = (8, 8, 1, PP)
    most = (1 << 31) - 1
    assert gpu.decode_chunks_plan(*prm, [8 * most])["items"] == most
    assert gpu.decode_chunks_plan(*prm, [8 * most, 1]) is None
    assert gpu.decode_chunks_plan(*prm, [8 * (most + 1)]) is None


@pytest.mark.parametrize("prm", [
    (0, 8, 128, PP), (33, 8, 128, PP), (8, 7, 128, PP | AEC_NOT_ENFORCE), (8, 8, 0, PP), (8, 8, 4097, PP),
    (8, 66, 16, PP | AEC_NOT_ENFORCE), (1, 8, 16, AEC_DATA_SIGNED), (6, 8, 16, AEC_RESTRICTED),
])
def test_what_check_params_refuses_the_plan_refuses(prm):
    assert gpu._lib().aec_gpu_check_params(C.byref(gpu.Params(*prm)), 0) != 0
    assert gpu.decode_chunks_plan(*prm, [1000, 2000]) is None
    assert gpu.decode_chunks_plan(*prm, []) is None
