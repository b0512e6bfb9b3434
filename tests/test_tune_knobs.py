"""The tuning build's knobs (libaec_amd/csrc/aec_tune.h) exist for tests, benches and scripts that compare variants: a
name read through tune() / tune_set() that none of them sets is a variant nothing tests, and a constant written the
long way.  Every name the sources read must be named under tests/ or in bench.py, and listed in aec_tune.h."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libaec_amd", "csrc")


def read(path):
    with open(path, errors="replace") as f:
        return f.read()


def test_every_knob_is_used_and_listed():
    names = set()
    for path in glob.glob(os.path.join(CSRC, "*")):
        if os.path.isfile(path):
            names |= set(re.findall(r'\btune(?:_set)?\(\s*"(\w+)"', read(path)))
    assert "AEC_IDX_SMALL" in names, "no tune() call found: has the pattern above gone stale?"
    users = [p for p in glob.glob(os.path.join(ROOT, "tests", "**", "*"), recursive=True)
             if os.path.isfile(p) and "__pycache__" not in p and "_build" not in p
             and os.path.abspath(p) != os.path.abspath(__file__)]
    text = "\n".join(read(p) for p in users + [os.path.join(ROOT, "bench.py")])
    unused = sorted(n for n in names if not re.search(r"\b%s\b" % re.escape(n), text))
    assert not unused, f"read by the sources, named by no test, bench or script: {unused}"
    listed = set(re.findall(r"^//   (\w+)", read(os.path.join(CSRC, "aec_tune.h")), flags=re.M))
    assert names <= listed, f"not in the list of aec_tune.h: {sorted(names - listed)}"
