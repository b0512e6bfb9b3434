"""aec_gpu_estimate_plan (include/aec_gpu.h; host arithmetic, no device): the sizes evaluated, the workspace and the
refusals, against a restatement in Python: one 16-bit record per block and size, pieces of 64 samples, every size's
records rounded up to 16 bytes."""
import ctypes as C

import pytest

import helpers
from helpers import AEC_DATA_3BYTE, AEC_DATA_MSB, AEC_DATA_PREPROCESS as PP, AEC_DATA_SIGNED, AEC_RESTRICTED

from libaec_amd import gpu

VALID = [(8, PP), (16, PP | AEC_DATA_MSB), (16, PP | AEC_DATA_SIGNED), (12, PP), (24, PP | AEC_DATA_3BYTE), (32, PP), (16, 0),
         (4, PP | AEC_RESTRICTED), (2, PP | AEC_RESTRICTED), (1, PP)]
VECTORS = [[128] * 4, [1] * 4, [3, 5, 7, 2], [4096] * 4, [0, 16, 0, 0], [5, 0, 0, 9], None]
SIZES = [0, 1, 2, 3, 63, 64, 65, 4096, 1 << 20, (1 << 20) + 7, 3 << 30]


def workspace(in_bytes, bps, flags, vec, rsi_all):
    samples = in_bytes // helpers.bytes_per_sample(bps, flags)
    pieces = (samples + 63) // 64
    total = 0
    for i in range(4):
        if (vec[i] if vec is not None else rsi_all):
            total += (pieces * (64 >> (3 + i)) * 2 + 15) // 16 * 16
    return total


@pytest.mark.parametrize("bps,flags", VALID)
def test_valid_sets_mask_and_workspace(bps, flags):
    for vec in VECTORS:
        for size in SIZES:
            plan = gpu.estimate_plan(bps, flags, vec, size, rsi_all=17)
            assert plan is not None, (vec, size)
            assert plan["evaluated"] == sum(1 << i for i in range(4) if (vec[i] if vec is not None else 17)), vec
            assert plan["workspace_bytes"] == workspace(size, bps, flags, vec, 17), (vec, size)


def test_records_are_under_half_a_byte_per_sample():
    plan = gpu.estimate_plan(16, PP, [128] * 4, 2 << 20)
    assert plan["workspace_bytes"] == (1 << 20) * 30 // 64       # 15 records of 2 bytes per piece of 64 samples


@pytest.mark.parametrize("bps,flags,vec,rsi_all", [
    (0, PP, None, 128), (33, PP, None, 128), (1, PP | AEC_DATA_SIGNED, None, 128), (6, PP | AEC_RESTRICTED, None, 128),
    (8, PP, [128, 128, 4097, 128], 128), (8, PP, [4097, 0, 0, 0], 128), (8, PP, [0, 0, 0, 0], 128),
    (8, PP, None, 0), (8, PP, None, 4097)])
def test_refused_sets(bps, flags, vec, rsi_all):
    assert gpu.estimate_plan(bps, flags, vec, 4096, rsi_all=rsi_all) is None


def test_a_size_that_is_not_asked_for_is_not_checked():
    """rsi[i] == 0 takes size i out: an RSI vector decides alone, p->rsi and p->block_size play no part"""
    assert gpu.estimate_plan(8, PP, [0, 0, 0, 4096], 4096, rsi_all=4097) == \
        {"evaluated": 8, "workspace_bytes": workspace(4096, 8, PP, [0, 0, 0, 4096], 0)}
    lib = gpu._lib()
    plan = gpu.EstimatePlan()
    for bs in (0, 8, 7, 1000):
        p = gpu.Params(8, bs, 17, PP)
        assert lib.aec_gpu_estimate_plan(C.byref(p), None, 4096, C.byref(plan)) == 1
        assert plan.evaluated == 15 and plan.pad == 0


def test_null_arguments():
    lib = gpu._lib()
    p = gpu.Params(8, 8, 128, PP)
    plan = gpu.EstimatePlan()
    assert lib.aec_gpu_estimate_plan(None, None, 4096, C.byref(plan)) == 0
    assert lib.aec_gpu_estimate_plan(C.byref(p), None, 4096, None) == 0
    assert lib.aec_gpu_estimate_plan(C.byref(p), None, 4096, C.byref(plan)) == 1


def test_the_async_call_refuses_before_it_touches_the_device():
    """parameter errors and NULL arguments come back from the host checks: no context, no device needed"""
    lib = gpu._lib()
    p = gpu.Params(8, 8, 128, PP)
    est = gpu.Estimate()
    assert lib.aec_gpu_estimate_async(None, C.byref(p), None, 0, None, C.byref(est), None) == helpers.AEC_CONF_ERROR
