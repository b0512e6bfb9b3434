#!/usr/bin/env python3
"""Generate the two stored tables of the narrow cases (tests/narrow_cases.py).  Run in the build container only.

tests/golden/narrow_chain.json: which schemes the index pass takes for the streams tests/test_gpu_narrow.py claims to
exercise -- host arithmetic of the library as it stands (aec_gpu_index_plan; for the shapes of tests/cross_scheme.py
--narrow also aec_gpu_index_scheme of the tuning build as its switches take the schemes away).  tests/test_narrow_emul.py
holds the library to it: a threshold that moves fails there, and this file is regenerated with the reason in the commit.

tests/golden/narrow_sz.json: two SZIP chunks of 1 MiB -- 1-bit pixels in blocks of 2 with scan lines of 128, 5-bit pixels in
blocks of 10 with scan lines of 1000 -- and what SZ_BufftoBuffCompress of the REFERENCE shim (src/sz_compat.c inside
oracle/_ref/libaec_ref.so) made of them: length and SHA-256 of its bytes (420 KB that do not compress), with the digest of
the input, which tests/narrow_cases.py: sz_chunks() generates again.  Data only."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import narrow_cases as N  # noqa: E402
from helpers import REF_SO  # noqa: E402
from libaec_amd import szip  # noqa: E402


def chains():
    env = dict(os.environ, AEC_AMD_LIB=os.path.join(ROOT, "libaec_amd", "lib", "tuning", "libaec.so.0"))
    out = subprocess.run([sys.executable, os.path.join(os.path.dirname(HERE), "narrow_cases.py"), "forced"], env=env,
                         capture_output=True, text=True, check=True)
    table = {"dispatch": N.dispatch_table(), "forced": json.loads(out.stdout)}
    for row in table["dispatch"]:
        assert row["chain"][0] == row["first_scheme"], row
    with open(N.GOLDEN_CHAINS, "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
    print(len(table["dispatch"]), "dispatch streams,", len(table["forced"]), "forced shapes")


def sz_vectors():
    ref = szip.bind(C.CDLL(REF_SO))
    rows = []
    for name, prm, data in N.sz_chunks():
        opts, bpp, ppb, pps = prm
        rc, comp = szip.compress(data, data.size * 2 + 4096, opts, bpp, ppb, pps, lib=ref)
        assert rc == 0, (name, rc)
        rc, dec = szip.decompress(comp, data.size, opts, bpp, ppb, pps, lib=ref)
        assert rc == 0 and dec == data.tobytes(), (name, rc, len(dec))
        rows.append({"name": name, "params": list(prm), "input_bytes": int(data.size),
                     "input_sha256": hashlib.sha256(data.tobytes()).hexdigest(), "stream_bytes": len(comp),
                     "stream_sha256": hashlib.sha256(comp).hexdigest()})
    with open(N.GOLDEN_SZ, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    print(len(rows), "SZ chunks,", sum(r["stream_bytes"] for r in rows), "stream bytes (digests stored)")


if __name__ == "__main__":
    chains()
    sz_vectors()
