"""k_place (libaec_amd/csrc/aec_enc.hip: the slots of the route that codes every block once, to their places in the
stream) at the borders of its rounds and groups of rounds: tests/place_rounds_cases.py has the input, whose runs have
every length the kernel can go wrong at, and the cases.  Every test is a child process on the tuning library with
AEC_ENC_LOCAL=1; the stream is compared byte for byte with the oracle's."""
import pytest

from test_gpu_encode_local import child

pytestmark = pytest.mark.gpu


def test_run_lengths_at_round_and_group_borders():
    """wavefronts of 8 segments: stream, RSI offsets, segment table and k_out exact, and the stream decodes to the input"""
    assert "place rounds ok: runs" in child(["place_rounds_cases.py", "runs"])


def test_other_run_lengths_and_buffer_edges():
    """the same input in wavefronts of 1 and of 32 segments, into a buffer of 0xFF, and with a capacity that ends in a run's middle
    round and one that ends with a run's first word"""
    assert "place rounds ok: again" in child(["place_rounds_cases.py", "again"])


def test_stream_longer_than_2_to_31_bits():
    """264 MiB of noise: run edges past bit 2^31 of the stream, against the analyze / scan / pack route, and decoded"""
    assert "place rounds ok: past" in child(["place_rounds_cases.py", "past"])
