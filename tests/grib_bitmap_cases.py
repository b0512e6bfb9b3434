"""GRIB2 section 6 bitmaps on the device (include/aec_gpu_grib.h, the *_bitmap_* calls): the case list shared by
tests/test_grib_bitmap_emul.py, tests/test_grib_bitmap_layout.py and tests/test_gpu_grib_bitmap.py.  Seeded; the masks are
packed by numpy.packbits; the model of what a pack leaves is grib_cases.pack_model / x_bytes of y[mask], of an unpack
grib_cases.dequantise scattered by NumPy.

T is the tile (the grid points a wavefront owns).  Every batch mixes the same list of grids of unequal size under one
template: sizes 1, 7, 8, 9, 63, 64, 65, T - 1, T, T + 1, 2T + 5 and 65T + 3 (66 tiles: two rounds of the scan) against
masks that are all ones, hold one point (the first, the last, point T), only the last point of every tile, a tile of zeros
in the middle, two tiles of zeros behind the last present point (the writer of the last block's padding is then not in the
last tile), alternating bits, random bits at densities 0.05, 0.5 and 0.95, and contiguous patches."""
import numpy as np

import grib_cases as gc

T = 1024
MISMATCH = 8
GRIDS = [(1, "ones"), (7, "random50"), (8, "alt"), (9, "first"), (63, "last"), (64, "random95"), (65, "random05"),
         (T - 1, "patches"), (T, "ones"), (T + 1, "at_T"), (T + 1, "last"), (2 * T + 5, "tile_last"), (2 * T + 5, "first"),
         (2 * T + 5, "random50"), (65 * T + 3, "zero_mid"), (65 * T + 3, "zero_tail2"), (65 * T + 3, "random50"),
         (65 * T + 3, "patches"), (2 * T + 5, "alt"), (T, "random05"), (65 * T + 3, "random95"), (9, "ones")]
# (nbits, block size, element type, first byte of the bitmaps, missing value of the unpack)
TEMPLATES = [(8, 8, np.float32, 0, 9999.0), (12, 32, np.float64, 1, float("nan")), (24, 32, np.float32, 3, float("nan")),
             (8, 32, np.float64, 3, 9999.0), (12, 8, np.float32, 1, 9999.0), (24, 8, np.float64, 0, float("nan"))]


def mask_of(kind, n, rng):
    m = np.zeros(n, bool)
    if kind == "ones":
        m[:] = True
    elif kind == "first":
        m[0] = True
    elif kind == "last":
        m[-1] = True
    elif kind == "at_T":
        m[T] = True
    elif kind == "tile_last":
        m[T - 1::T] = True
    elif kind == "alt":
        m[1::2] = True
    elif kind.startswith("random"):
        m = rng.random(n) < int(kind[6:]) / 100.0
        m[int(rng.integers(0, n))] = True                      # (never without a present point)
    elif kind == "patches":                                     # a land-sea shape: runs of 3 .. 400 points, about 30 % missing
        at, sea = 0, True
        while at < n:
            run = int(rng.integers(3, 400 if sea else 170))
            m[at:at + run] = sea
            at, sea = at + run, not sea
        m[n // 2] = True
    elif kind == "zero_mid":                                    # tile 31 without a present point
        m = rng.random(n) < 0.5
        m[31 * T:32 * T] = False
    elif kind == "zero_tail2":                                  # the last present point lies in tile 62; two more whole tiles
        m = rng.random(n) < 0.5                                 # and the 3 points of the last one behind it are zeros
        m[63 * T - 7:] = False
        m[63 * T - 8] = True
    else:
        raise ValueError(kind)
    return m


def junk(dtype):
    """what absent points hold"""
    out = [np.nan, np.inf, -np.inf, 9999.0]
    return out + [1e300] if dtype == np.float64 else out


def _batches():
    out = []
    for k, (nbits, bs, dtype, bm0, missing) in enumerate(TEMPLATES):
        rng = np.random.default_rng(6000 + k)
        grids, masks, values = [], [], []
        for i, (n, kind) in enumerate(GRIDS):
            m = mask_of(kind, n, rng)
            y = gc._smooth(rng, n, dtype).astype(dtype)
            g = y.copy()
            g[~m] = np.resize(np.array(junk(dtype), dtype), int((~m).sum()))
            grids.append(np.ascontiguousarray(g))
            masks.append(m)
            values.append(np.ascontiguousarray(y[m]))
        name = f"bm{nbits}_bs{bs}_{'f4' if dtype == np.float32 else 'f8'}"
        b = gc._batch(name, nbits, gc.PP, bs, 128, dtype, values, [gc.D_CYCLE[i % 3] for i in range(len(GRIDS))])
        out.append(dict(b, grids=grids, masks=masks, bm0=bm0, missing=missing, bases=["aligned" if i % 2 else "elem" for i in range(len(GRIDS))]))
    return out


_ALL = []


def batches():
    """dicts as grib_cases.batches() gives them (fields = the PRESENT values of every grid, so grib_cases.model_of(b) is the
    model of the pack), with grids (the whole grids, junk at the absent points), masks (bool), bm0, missing and bases"""
    if not _ALL:
        _ALL.extend(_batches())
    return _ALL


def bitmaps(b):
    """(the bitmaps of a batch back to back from byte bm0 -- neighbours touch, so they begin on any byte --, their offsets)"""
    parts = [np.packbits(m) for m in b["masks"]]
    offs = np.concatenate([[b["bm0"]], b["bm0"] + np.cumsum([p.size for p in parts])]).astype(np.uint64)
    return np.concatenate([np.zeros(b["bm0"], np.uint8)] + parts), offs[:-1]


def grid_placement(b):
    """where the whole grids lie: grib_cases.edge_placement over them (on a 16-byte boundary / one element behind one)"""
    return gc.edge_placement(dict(b, fields=b["grids"]))


def tile_bases(mask):
    """the NumPy prefix sum: ones in front of every tile"""
    tiles = (mask.size + T - 1) // T
    per = np.add.reduceat(mask.astype(np.uint64), np.arange(0, mask.size, T))
    assert per.size == tiles
    return np.concatenate([[0], np.cumsum(per)[:-1]]).astype(np.uint64)


def expanded(b, i, model, missing):
    """the grid an unpack leaves: grib_cases.dequantise scattered by NumPy, the bits of (T)missing elsewhere"""
    R, E, st, x = model[i]
    out = np.full(b["masks"][i].size, missing, b["dtype"])
    out[b["masks"][i]] = gc.dequantise(x, R, E, b["D"][i], b["dtype"])
    return out


def build_grids(b, missing):
    """the grids with `missing` at the absent points (what aec_gpu_grib_bitmap_async reads)"""
    out = []
    for g, m in zip(b["grids"], b["masks"]):
        g = g.copy()
        g[~m] = missing
        out.append(g)
    return out
