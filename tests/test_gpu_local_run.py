"""k_encode_local's walk over a run on the device, against the oracle: tests/local_run_cases.py has the cases, the inputs
and what every input has to drive.  Every device test is a child process on the tuning library with AEC_ENC_LOCAL=1, which
takes the route that codes every block once at any size."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import ROOT, oracle_encode
import local_run_cases as cases

TUNING = os.path.join(ROOT, "libaec_amd", "lib", "tuning", "libaec.so.0")
IDS = [f"rsi{c[0]}-{c[1]}seg" for c in cases.CASES]


@pytest.mark.parametrize("index", range(len(cases.CASES)), ids=IDS)
def test_drive_inputs_miss_merge_and_fall_back(index):
    """(no device) the model of the k chain is the oracle's, and by it the "drive" input of every case and run length has
    a run coded again -- up to a segment that stays and from behind its first segment wherever the shape has such runs --
    an uncompressed block and a zero run across a segment end"""
    case = cases.CASES[index]
    for spw in case[2]:
        name, data, _ = next(cases.inputs(case, spw))
        data = np.ascontiguousarray(data, dtype=np.uint8)
        assert data.size == cases.blocks_of(case) * cases.BS * 2 and cases.blocks_of(case) % 64 == cases.LAST
        rc, _, trace, _, _ = oracle_encode(data, *cases.prm_of(case), want_trace=True)
        assert rc == 0
        print(case, spw, cases.properties(case, spw, data, trace))


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(cases.CASES)), ids=IDS)
def test_streams_tables_and_decode(index):
    e = dict(os.environ)
    for name in ("AEC_ENC_LOCAL", "AEC_ENC_LOCAL_SPW", "AEC_ENC_LOCAL_GUESS", "AEC_AMD_LIB"):
        e.pop(name, None)
    assert os.path.exists(TUNING)
    e["AEC_AMD_LIB"] = TUNING
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "local_run_cases.py"), "run", str(index)], env=e,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "local run ok" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])
