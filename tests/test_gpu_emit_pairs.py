"""The small-block emitter on sample pairs on the device, against the oracle: tests/emit_pairs_cases.py has the cases and
the classes of blocks every input must hold.  Every test is a child process on the tuning library with AEC_ENC_LOCAL=1,
which takes the route that codes every block once at any size; each case runs the analyze / scan / pack route as well."""
import os
import subprocess
import sys

import pytest

from helpers import ROOT
import emit_pairs_cases as cases

TUNING = os.path.join(ROOT, "libaec_amd", "lib", "tuning", "libaec.so.0")


def test_inputs_hold_every_class():
    """(no device) the seeds chosen pass the refusal: read off the oracle's trace, every input holds every class"""
    for prm in cases.SHAPES:
        for what, data in cases.inputs(prm):
            cases.checked_trace(prm, what, data)


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(cases.SHAPES)), ids=["-".join(str(x) for x in p[:3]) for p in cases.SHAPES])
def test_streams_tables_and_decode(index):
    e = dict(os.environ)
    for name in ("AEC_ENC_LOCAL", "AEC_ENC_LOCAL_SPW", "AEC_ENC_LOCAL_GUESS", "AEC_AMD_LIB"):
        e.pop(name, None)
    assert os.path.exists(TUNING)
    e["AEC_AMD_LIB"] = TUNING
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "emit_pairs_cases.py"), "run", str(index)], env=e,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "emit pairs ok" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])
