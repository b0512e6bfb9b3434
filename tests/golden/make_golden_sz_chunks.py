#!/usr/bin/env python3
"""Generate tests/golden/sz_chunks_vectors.npz with the REFERENCE SZIP shim (src/sz_compat.c inside
oracle/_ref/libaec_ref.so): the unequal batches of tests/sz_chunks_cases.py, chunk by chunk.  Run in the build
container only.  Data only: parameters, sizes, input bytes and the bytes SZ_BufftoBuffCompress produced.

Only whole pixels are coded (include/aec_gpu_sz.h; sz_abi.cpp).  The reference, handed a trailing fraction of a pixel,
copies the fraction's bytes into the last scan line and repeats a "last pixel" that starts in the middle of one
(src/sz_compat.c:82-93); with byte planes it reads them from a buffer it never wrote (src/sz_compat.c:137-163).  A chunk
is therefore given to the reference without its fraction, which is what the product codes of it; the stored input keeps
the fraction."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from helpers import REF_SO  # noqa: E402
from libaec_amd import szip  # noqa: E402
from sz_chunks_cases import GOLDEN, batches, unit_of  # noqa: E402


def main():
    ref = szip.bind(C.CDLL(REF_SO))
    names, params, n_chunks, sizes, lens, inputs, outputs = [], [], [], [], [], [], []
    for name, prm, batch_sizes, chunks in batches():
        opts, bpp, ppb, pps = prm
        for size, chunk in zip(batch_sizes, chunks):
            data = np.ascontiguousarray(chunk).view(np.uint8).reshape(-1)
            assert data.size == size, (name, size)
            whole = size - size % unit_of(bpp)
            coded = data[:whole]
            rc, comp = szip.compress(coded, size * 2 + 4096, opts, bpp, ppb, pps, lib=ref)
            assert rc == 0, (name, size, rc)
            rc, dec = szip.decompress(comp, size, opts, bpp, ppb, pps, lib=ref)
            assert rc == 0 and dec[:whole] == data[:whole].tobytes(), (name, size, rc, len(dec))
            sizes.append(size)
            lens.append(len(comp))
            inputs.append(data)
            outputs.append(np.frombuffer(comp, np.uint8))
        names.append(name)
        params.append(prm)
        n_chunks.append(len(batch_sizes))
    in_off = np.cumsum([0] + [sum(sizes[sum(n_chunks[:b]):sum(n_chunks[:b + 1])]) for b in range(len(names))]).astype(np.uint64)
    out_off = np.cumsum([0] + [sum(lens[sum(n_chunks[:b]):sum(n_chunks[:b + 1])]) for b in range(len(names))]).astype(np.uint64)
    np.savez_compressed(GOLDEN, names=np.array(names), params=np.array(params, dtype=np.int32),
                        n_chunks=np.array(n_chunks, dtype=np.uint64), sizes=np.array(sizes, dtype=np.uint64),
                        stream_bytes=np.array(lens, dtype=np.uint64), in_off=in_off, out_off=out_off,
                        inputs=np.concatenate(inputs), outputs=np.concatenate(outputs))
    print(len(names), "batches,", len(sizes), "chunks,", int(in_off[-1]), "input bytes,", int(out_off[-1]), "stream bytes,",
          os.path.getsize(GOLDEN), "bytes on disk")


if __name__ == "__main__":
    main()
