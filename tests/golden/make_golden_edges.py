#!/usr/bin/env python3
"""Write tests/golden/predictor_edges.json with the REFERENCE libaec (oracle/_ref/libaec_ref.so, compiled by
oracle/Makefile where the reference's tree exists): the length and the SHA-256 of the stream its aec_buffer_encode
produces for every case of tests/predictor_edges.py.  The vectors themselves are generated, not stored; the hashes pin
them to the reference on machines that have no oracle/_ref.

    python tests/golden/make_golden_edges.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import helpers as H  # noqa: E402
import predictor_edges as E  # noqa: E402


def main():
    assert H.have_ref(), "the compiled reference is needed"
    out = {}
    for family, cfg in E.cases():
        x, data = E.vector(family, cfg)
        bps, bs, rsi, flags = cfg
        rc, enc = H.ref_encode(data, bps, bs, rsi, flags)
        assert rc == H.AEC_OK, (family, cfg, rc)
        nblk = (x.size + bs - 1) // bs
        rc, dec = H.ref_decode(enc, bps, bs, rsi, flags, nblk * bs * H.bytes_per_sample(bps, flags))
        assert rc == H.AEC_OK and dec == E.expected_decode(x, cfg), (family, cfg, rc)
        out[E.case_id(family, cfg)] = E.digest(enc)
    with open(E.GOLDEN_JSON, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(out), "cases")


if __name__ == "__main__":
    main()
