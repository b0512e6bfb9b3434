"""Cases of tests/test_gpu_sz_device.py that tests/test_sz_layout.py checks on the CPU (the layout call takes them)."""
import numpy as np

MSB, NN, RAW = 16, 32, 128          # SZ_MSB_OPTION_MASK, SZ_NN_OPTION_MASK, SZ_RAW_OPTION_MASK
SWEEP_SEED, SWEEP_CASES = 20, 30


def sweep_cases():
    """30 random parameter sets: bits per pixel in {1..16, 24, 32, 64}, pixels per block even in 2..32, pixels per scan
    line 1..2000, NN on or off, MSB or LSB, 1..12 chunks of at most 64 KiB (whole pixels, any number of them)"""
    rng = np.random.default_rng(SWEEP_SEED)
    widths = list(range(1, 17)) + [24, 32, 64]
    for i in range(SWEEP_CASES):
        # (every third draw from the wide pixels, which the 19 widths would rarely give)
        bpp = int(rng.choice([24, 32, 64])) if i % 3 == 2 else int(rng.choice(widths))
        ppb = 2 * int(rng.integers(1, 17))
        pps = int(rng.integers(1, 2001))
        opts = RAW | (NN if rng.random() < 0.5 else 0) | (MSB if rng.random() < 0.5 else 0)
        unit = bpp // 8 if bpp in (32, 64) else (4 if bpp > 16 else (2 if bpp > 8 else 1))
        pixels = int(rng.integers(1, 65536 // unit + 1))
        if rng.random() < 0.3:
            pixels = max(1, pixels // (pps * 4) * (pps * 4))      # some whole lines, some whole lines of whole quads
        yield dict(opts=opts, bpp=bpp, ppb=ppb, pps=pps, n=int(rng.integers(1, 13)), chunk_bytes=pixels * unit, seed=i)


def chunk_data(case):
    """smooth data of the pixel width with some noise, as n chunks of chunk_bytes"""
    rng = np.random.default_rng(100 + case["seed"])
    n, size, bpp = case["n"], case["chunk_bytes"], case["bpp"]
    unit = bpp // 8 if bpp in (32, 64) else (4 if bpp > 16 else (2 if bpp > 8 else 1))
    count = n * size // unit
    walk = np.cumsum(rng.integers(-3, 4, size=count)).astype(np.int64) + (1 << (min(bpp, 62) - 1))
    vals = (walk & ((1 << min(bpp, 63)) - 1)).astype(np.uint64)
    raw = np.zeros((count, unit), dtype=np.uint8)
    for b in range(unit):
        shift = 8 * (unit - 1 - b) if case["opts"] & MSB else 8 * b
        raw[:, b] = (vals >> np.uint64(shift)) & np.uint64(0xFF)
    return raw.reshape(n, size)
