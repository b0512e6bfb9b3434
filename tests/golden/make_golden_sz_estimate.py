#!/usr/bin/env python3
"""Generate tests/golden/sz_estimate.json with the REFERENCE SZIP shim (src/sz_compat.c inside
oracle/_ref/libaec_ref.so): for every case of tests/sz_estimate_cases.py, every chunk and every pixels-per-block asked,
the LENGTH of the stream SZ_BufftoBuffCompress made.  Run in the build container only.  Lengths only: the inputs are
made again from their seeds by the tests.

As in make_golden_sz_chunks.py a chunk is given to the reference without its trailing fraction of a pixel, which is what
the product codes of it."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from helpers import REF_SO  # noqa: E402
from libaec_amd import szip  # noqa: E402
from sz_estimate_cases import GOLDEN, all_cases, unit_of  # noqa: E402


def main():
    ref = szip.bind(C.CDLL(REF_SO))
    out, streams = {}, 0
    for name, opts, bpp, pps, chunks in all_cases():
        rows = []
        for chunk in chunks:
            data = np.ascontiguousarray(chunk).view(np.uint8).reshape(-1)
            coded = data[:data.size - data.size % unit_of(bpp)]
            row = [None] * 4
            for i in range(4):
                if not pps[i]:
                    continue
                rc, comp = szip.compress(coded, 2 * data.size + 8 * pps[i] + 4096, opts, bpp, 8 << i, pps[i], lib=ref)
                assert rc == 0, (name, data.size, i, rc)
                rc, dec = szip.decompress(comp, coded.size, opts, bpp, 8 << i, pps[i], lib=ref)
                assert rc == 0 and dec == coded.tobytes(), (name, data.size, i, rc)
                row[i] = len(comp)
                streams += 1
            rows.append(row)
        out[name] = rows
    with open(GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(len(out), "cases,", streams, "streams,", os.path.getsize(GOLDEN), "bytes on disk")


if __name__ == "__main__":
    main()
