"""The predictor shortcuts of the kernels at their exact thresholds (tests/predictor_edges.py: the vectors, the model that
shows they sit there, and gpu_check, which takes one vector through the device encoder, the table decode on the lane or
the wave kernel and on the generic kernel, the segment decode, the bare decode by segments and the libaec ABI, whole and
cut inside the clipping blocks).  Expected bytes are the oracle's, pinned to the reference by the hashes in
tests/golden/predictor_edges.json; tests/test_predictor_edges.py checks on the CPU that every vector reaches the
conditions it is meant for."""
import pytest

import predictor_edges as E

pytestmark = pytest.mark.gpu


def _ids(family):
    return [E.case_id(family, c) for c in E.CONFIGS[family]]


@pytest.mark.parametrize("cfg", E.CONFIGS["tight_pairs"], ids=_ids("tight_pairs"))
def test_tight_pairs(cfg):
    """steps that equal the room (two-sided) and steps one beyond it (one-sided), on every sample slot and border"""
    assert "encode" in E.gpu_check("tight_pairs", cfg)


@pytest.mark.parametrize("cfg", E.CONFIGS["wave_layout"], ids=_ids("wave_layout"))
def test_wave_layout(cfg):
    """segments whose every stretch fits, one of them tightly, and the same with one stretch one beyond: lane 0, lane 63,
    a later chunk round, the last stretch"""
    assert "encode" in E.gpu_check("wave_layout", cfg)


@pytest.mark.parametrize("cfg", E.CONFIGS["inactive_lanes"], ids=_ids("inactive_lanes"))
def test_inactive_lanes(cfg):
    """short last segments that fit while the blocks the idle lanes read do not"""
    assert "encode" in E.gpu_check("inactive_lanes", cfg)


@pytest.mark.parametrize("cfg", E.CONFIGS["block_ladders"], ids=_ids("block_ladders"))
def test_block_ladders(cfg):
    """blocks whose residuals sum to the room and to one more, amid other ladders and alone among blocks that fit"""
    assert "encode" in E.gpu_check("block_ladders", cfg)


@pytest.mark.parametrize("cfg", E.CONFIGS["segment_edges"], ids=_ids("segment_edges"))
def test_segment_edges(cfg):
    """RSIs of which one segment sits on an end of the interval its running sum holds for, or one beyond it, in streams
    long enough that the index pass leaves the segment starts and the bare decode sums per segment"""
    ran = E.gpu_check("segment_edges", cfg)
    assert "bare decode by segments" in ran and "bare decode by segments, index record" in ran, ran


@pytest.mark.parametrize("cfg", E.CONFIGS["extremes"], ids=_ids("extremes"))
def test_extremes(cfg):
    """the largest residual throughout; 32-bit blocks whose sum wraps; residuals of 2^26 - 1 and 2^26"""
    assert "encode" in E.gpu_check("extremes", cfg)


@pytest.mark.parametrize("cfg", E.CONFIGS["every_pair"], ids=_ids("every_pair"))
def test_every_pair(cfg):
    """every ordered pair of sample values of 3, 5, 7 and 8 bits"""
    assert "encode" in E.gpu_check("every_pair", cfg)


@pytest.mark.parametrize("cfg", E.CONFIGS["every_block_clips"], ids=_ids("every_block_clips"))
def test_every_block_clips(cfg):
    """260 and more consecutive blocks with a clipping step each: the wave kernel corrects lane after lane"""
    assert "encode" in E.gpu_check("every_block_clips", cfg)
