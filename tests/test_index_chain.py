"""The CHAIN of schemes the index pass of a bare stream enqueues (libaec_amd/csrc/aec_idx.hip: index_chain), as
aec_gpu_index_plan reports it -- host arithmetic, pinned here without a GPU.  The launch, aec_gpu_index_scheme and the two
workspace sizes all read the one list index_chain builds, so this file pins all of them at once.

Cases: every row of tests/test_index_scheme.py as the plain pass, with segment starts wanted, as a piece of a longer
stream (aec_gpu_set_index_piece), and -- rows that start on an RSI whose RSIs have more than one block -- as a walk that
resumes inside an RSI (start block 1).

tests/golden/index_chain.json holds, per case, what the commit BEFORE the chain existed returned: the first scheme
(aec_gpu_index_scheme) and the two workspace sizes (index_workspace_bytes, index_workspace_bytes_large; recorded through
a throw-away export of the two functions).  They must not move by a byte.

The lists of scheme ids below are that commit's launch_index read branch by branch (and checked against a dry run of
it that recorded which launch_index_* it called).  The serial walk that the chains and the every-bit scheme enqueue
behind themselves is part of those schemes and not listed.  Which branch gives which list:

  [4]        the every-bit scheme first: it runs alone (never with segment starts wanted where the decoder takes them,
             never for a piece)
  [5, ...]   regions in front (large preprocessed streams); whatever would run without them is enqueued behind
  [1]        the 64 agreeing chains (mode 0) with the serial walker behind them
  [1, 4]     entries by plausibility (mode 1), then the every-bit scheme piece by piece (streams of up to 2^28 bits, of
             2^25 where RSIs have 64 blocks and more; not for a piece)
  [1, 1, 3]  mode 1 without that fallback: the 64 agreeing chains where RSIs are short (lock_plan_alt), then the trunk
  [1, 3]     the same where RSIs are too long for the agreeing chains
  [2, 4]     window tables of ONE span with nothing in front: the walker may give up, the every-bit scheme behind takes
             the stream (streams of up to 2^24 bits; not for a piece)
  [2]        window tables otherwise
  [3]        the trunk
  [0]        the serial walk alone
"""
import json
import os

import pytest

from libaec_amd import gpu
from test_index_scheme import CASES

SERIAL, LOCKED, TABLES, TRUNK, EVERY_BIT, REGIONS = range(6)
VARIANTS = ("plain", "segments", "piece", "resumed")

# per row of test_index_scheme.CASES, in its order: the chain of the plain pass, with segment starts, as a piece, resumed
# inside an RSI (None: the row resumes already, or its RSIs have one block)
CHAINS = [
    ([4], [4], [1], [4]),                       # a 64 KiB chunk, scan lines of 32 pixels (no segment decode for this shape)
    ([4], [4], [1], None),                      # the same, resumed
    ([4], [4], [3], [4]),                       # AEC_PAD_RSI: neither chains nor tables
    ([4], [4], [2], [4]),                       # the 8-bit SZIP shape, 64 KiB
    ([2, 4], [2, 4], [2], [2, 4]),              # the 8-bit SZIP shape, 1 MiB
    ([5, 2], [5, 2], [5, 2], [5, 2]),           # config 2, 1 GiB: regions, then window tables
    ([2, 4], [2, 4], [2], [2, 4]),              # config 2, 4 MiB
    ([4], [3], [3], [4]),                       # config 3, 1 MiB: segments are decoded for this shape, so no scheme 4
    ([3], [3], [3], [3]),                       # config 3, 1 GiB
    ([5, 3], [5, 3], [5, 3], [5, 3]),           # config 3, 4 GiB: regions, then the trunk
    ([4], [4], [1, 3], [4]),                    # the sample shape, 1 MiB
    ([1, 3], [1, 3], [1, 3], [1, 3]),           # the sample shape, 1 GiB: by plausibility (beyond 2^25 bits no every-bit
                                                # pieces behind RSIs of 256 blocks), then the trunk
    ([1], [1], [1], [1]),                       # 16 MiB of 8-bit data, rsi 32
    ([1], [1], [1], [1]),                       # ... rsi 33
    ([2], [2], [2], [2]),                       # ... rsi 48
    ([2], [2], [2], [2]),                       # config 2, 256 MiB
    ([1, 4], [1, 4], [1, 1, 3], [1, 1, 3]),     # 16 MiB of 16-bit data, rsi 32 (resumed: more than one every-bit piece
                                                # cannot begin inside an RSI)
    ([4], [4], [1, 3], [1, 3]),                 # 4 MiB of the sample shape
    ([1, 3], [1, 3], [1, 3], [1, 3]),           # 8 MiB of the sample shape
    ([4], [4], [3], [3]),                       # 16 MiB without the preprocessor
    ([3], [3], [3], [3]),                       # 16 MiB of 8-bit data without the preprocessor, rsi 128
    ([4], [4], [1, 1, 3], None),                # 1 MiB with rsi 1
    ([1, 4], [1, 4], [1, 1, 3], None),          # 16 MiB with rsi 1
    ([2], [2], [2], [2]),                       # 64 MiB of 8-bit noise
    ([5, 1, 3], [5, 1, 3], [5, 1, 3], [5, 1, 3]),   # the same with the ABI's hint: regions, by plausibility, the trunk
    ([3], [3], [3], [3]),                       # 64 MiB of 16-bit noise
    ([0], [0], [0], [0]),                       # nothing to index
]

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "index_chain.json")) as _f:
    GOLDEN = {(g["name"], g["variant"]): g for g in json.load(_f)}

PARAMS = [(row, variant, chain) for row, chains in zip(CASES, CHAINS) for variant, chain in zip(VARIANTS, chains)
          if chain is not None]


def test_the_table_covers_every_row_and_the_golden_file_every_case():
    assert len(CHAINS) == len(CASES)
    assert sorted(GOLDEN) == sorted((row[0], variant) for row, variant, _ in PARAMS)
    for row, chains in zip(CASES, CHAINS):
        # (the rows that get no resumed variant are exactly those that cannot have one more)
        assert (chains[3] is None) == (row[7] != 0 or row[3] == 1), row[0]


@pytest.mark.parametrize("row,variant,chain", PARAMS, ids=[f"{r[0]} [{v}]" for r, v, _ in PARAMS])
def test_index_chain(row, variant, chain):
    name, bps, bs, rsi, flags, nbytes, hint, start_block, scheme = row
    g = GOLDEN[(name, variant)]
    assert (g["bits_per_sample"], g["block_size"], g["rsi"], g["flags"], g["in_bytes"], g["rsi_bits"]) == \
        (bps, bs, rsi, flags, nbytes, hint)
    if variant == "resumed":
        start_block = 1
    segments, piece = variant == "segments", variant == "piece"
    assert (g["start_block"], g["want_segments"], g["piece"]) == (start_block, int(segments), int(piece))
    ids, asked, large, used = gpu.index_plan(bps, bs, rsi, flags, nbytes, hint, start_block, segments, piece)
    print(name, variant, ids, asked, large, used)
    # what the commit before returned, to the byte
    assert gpu.index_scheme(bps, bs, rsi, flags, nbytes, hint, start_block) == g["first_scheme"]
    assert asked == g["workspace_bytes"]
    assert large == g["workspace_bytes_large"]
    # the whole chain
    assert ids == chain, (name, variant, [gpu.INDEX_SCHEMES[i] for i in ids])
    if variant in ("plain", "resumed"):
        assert ids[0] == g["first_scheme"]
    if variant == "plain":
        assert ids[0] == scheme
    # with the workspace the pass asks for on offer, the stages lie inside it
    assert used <= asked, (name, variant, used, asked)
    # ... and a pass that is handed nothing walks serially
    if nbytes:
        assert gpu.index_plan(bps, bs, rsi, flags, nbytes, hint, start_block, segments, piece, ws_bytes=1)[0] == [SERIAL]
