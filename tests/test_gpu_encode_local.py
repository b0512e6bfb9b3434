"""The encoder route that codes every block once (libaec_amd/csrc/aec_enc_local.h: k_encode_local, k_encode_redo,
k_place) on the device, against the oracle: tests/enc_local_cases.py has the cases.  Every test is a child process on
the tuning library with AEC_ENC_LOCAL=1, which takes the route at any size, and AEC_ENC_LOCAL_SPW segments per wavefront;
the last one runs the library as shipped at its threshold."""
import os
import subprocess
import sys

import pytest

from helpers import ROOT

pytestmark = pytest.mark.gpu

TUNING = os.path.join(ROOT, "libaec_amd", "lib", "tuning", "libaec.so.0")


def child(args, env=None, tuning=True):
    e = dict(os.environ)
    for name in ("AEC_ENC_LOCAL", "AEC_ENC_LOCAL_SPW", "AEC_ENC_LOCAL_GUESS", "AEC_AMD_LIB"):
        e.pop(name, None)
    if tuning:
        assert os.path.exists(TUNING)
        e["AEC_AMD_LIB"] = TUNING
    e.update(env or {})
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", *args[:1]), *args[1:]], env=e, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    return out.stdout


@pytest.mark.parametrize("spw", [1, 8])
def test_sizes_and_data(spw):
    """one block to 33 wavefronts of random walk, zeros, a constant, noise and islands in zeros (several wavefronts in
    one word of the stream), for the three shapes that take the route, RSIs of one block, and a shape that keeps the
    old kernels"""
    assert "encode local ok: sweep" in child(["enc_local_cases.py", "sweep", str(spw)])


@pytest.mark.parametrize("spw", [1, 8])
def test_plateau_data_misses_and_is_exact(spw):
    """data on which half of the wavefronts miss whatever the guess: guess 0, guess 31 and the built-in rule"""
    assert "encode local ok: plateau" in child(["enc_local_cases.py", "plateau", str(spw)])


@pytest.mark.parametrize("spw", [1, 8])
def test_buffer_edges(spw):
    """an output buffer of 0xFF, and a capacity short of the stream"""
    assert "encode local ok: edges" in child(["enc_local_cases.py", "edges", str(spw)])


def test_predictor_edges_on_the_route():
    """tests/predictor_edges.py once more with the route forced on: it shares the feeder and its shortcuts"""
    out = child(["predictor_edges.py"], env={"AEC_ENC_LOCAL": "1"})
    assert "predictor edges ok" in out


def test_threshold_of_the_shipped_library():
    """the library as shipped one segment below the size from which it takes the route, and at it"""
    assert "encode local ok: threshold" in child(["enc_local_cases.py", "threshold"], tuning=False)
