#!/usr/bin/env python3
"""Write tests/golden/foreign_predictor.json with the REFERENCE libaec (oracle/_ref/libaec_ref.so, compiled by
oracle/Makefile where the reference's tree exists): for every case of tests/foreign_predictor.py the length and the
SHA-256 of the stream (generated, not stored: the hash says that a machine generates the same one) and of the bytes the
reference's aec_buffer_decode returns for it, with AEC_OK.  The hashes pin the oracle to the reference on machines that
have no oracle/_ref.

    python tests/golden/make_golden_foreign.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import helpers as H  # noqa: E402
import foreign_predictor as F  # noqa: E402


def main():
    assert H.have_ref(), "the compiled reference is needed"
    out = {}
    todo = [(F.case_id(f, c), c, F.vector(f, c)["stream"], None) for f, c in F.cases()]
    todo.append(("issue", F.ISSUE_CFG, F.ISSUE_STREAM, len(F.ISSUE_SAMPLES)))
    for name, cfg, stream, nsamp in todo:
        bps, bs, rsi, flags = cfg
        if nsamp is None:
            nsamp = F.vector(*next((f, c) for f, c in F.cases() if F.case_id(f, c) == name))["nblk"] * bs
        rc, dec = H.ref_decode(stream, bps, bs, rsi, flags, nsamp * H.bytes_per_sample(bps, flags))
        assert rc == H.AEC_OK and len(dec) == nsamp * H.bytes_per_sample(bps, flags), (name, rc, len(dec))
        out[name] = {"stream": F.digest(stream), "decoded": F.digest(dec)}
    with open(F.GOLDEN_JSON, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(out), "cases")


if __name__ == "__main__":
    main()
