#!/usr/bin/env python3
"""tests/resusage_compare.py with the scalar spills in the table: per instantiation of the encoder's and the decoder's
kernels in two source trees, SGPRs, SGPR spills, VGPRs, AGPRs, scratch, LDS and occupancy from the compiler's
resource-usage remarks.
    python tests/resusage_spills.py <parent tree>/libaec_amd/csrc <this tree>/libaec_amd/csrc"""
import contextlib
import io

import resusage_compare as rc

rc.KEYS = ["TotalSGPRs", "SGPRs Spill", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
           "Occupancy [waves/SIMD]"]
rc.UNITS = [u for u in rc.UNITS if u[1] != "aec_idx.hip"]
rc.without_flag = lambda name: (name, False)      # (both trees have the same template parameters)

if __name__ == "__main__":
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rc.main()
    lines = out.getvalue().splitlines()
    lines[0] = "columns: sgpr sgpr-spills vgpr agpr scratch(bytes/lane) lds(bytes/block, static) occupancy(waves/SIMD)"
    print("\n".join(lines))
