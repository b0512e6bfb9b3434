#!/usr/bin/env python3
"""Generate tests/golden/grib_vectors.npz: the fields of tests/grib_cases.py (among them the contraction witnesses, found
there with exact rational arithmetic), the model's X of every field, and the stream the REFERENCE's aec_buffer_encode
(oracle/_ref/libaec_ref.so) makes of each X.  Run in the build container only.  Data only: parameters, sizes, the fields'
values, X and the bytes the reference produced.  A field whose status says bad (a NaN, an Inf) has neither X nor stream."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import grib_cases as gc  # noqa: E402
from helpers import ref_decode, ref_encode  # noqa: E402


def main():
    names, tmpl, elem, n_fields, n_values, status, lens = [], [], [], [], [], [], []
    vals = {4: [], 8: []}
    xs, streams = [], []
    for b in gc.batches():
        nbits, options, bs, rsi = b["tmpl"]
        flags = gc.coder_flags(options, for_encode=False)
        for f, (R, E, st, x) in zip(b["fields"], gc.model_of(b)):
            vals[b["elem"]].append(f)
            n_values.append(f.size)
            status.append(st)
            if x is None:
                lens.append(0)
                continue
            data = gc.x_bytes(x, nbits, x.size)
            rc, enc = ref_encode(data, nbits, bs, rsi, flags)
            assert rc == 0, (b["name"], rc)
            rc, dec = ref_decode(enc, nbits, bs, rsi, flags, gc.room(x.size, bs, nbits))
            assert rc == 0 and dec[:data.size] == data.tobytes(), (b["name"], rc)
            xs.append(x)
            streams.append(np.frombuffer(enc, np.uint8))
            lens.append(len(enc))
        names.append(b["name"])
        tmpl.append(b["tmpl"])
        elem.append(b["elem"])
        n_fields.append(len(b["fields"]))
    np.savez_compressed(gc.GOLDEN, names=np.array(names), tmpl=np.array(tmpl, dtype=np.int32), elem=np.array(elem, dtype=np.int32),
                        n_fields=np.array(n_fields, dtype=np.uint64), n_values=np.array(n_values, dtype=np.uint64),
                        status=np.array(status, dtype=np.uint32), stream_bytes=np.array(lens, dtype=np.uint64),
                        values_f4=np.concatenate(vals[4]), values_f8=np.concatenate(vals[8]), x=np.concatenate(xs),
                        streams=np.concatenate(streams))
    print(len(names), "batches,", len(n_values), "fields,", int(sum(n_values)), "values,", int(sum(lens)), "stream bytes,",
          os.path.getsize(gc.GOLDEN), "bytes on disk")


if __name__ == "__main__":
    main()
