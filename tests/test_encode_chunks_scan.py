"""The segmented three-phase scan of aec_gpu_encode_chunks_async (libaec_amd/csrc/aec_chunks.h) on the CPU:
tests/emul/chunks_emul.cpp runs the functions the kernels k_chunks_reduce / k_chunks_bases / k_chunks_apply are loops over,
tile by tile and thread by thread, on random (bits, clamp) per segment; the chunks' bases, every segment's start bit and
carried k, the RSI table and the per-wave table must be what a plain loop over the chunks gives.  The words and bytes the
scan clears are checked against the rules the pack kernel relies on: the word every wave's first segment starts in, every
chunk's open last word plus one, the byte of every empty chunk."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
EMUL_SO = os.path.join(EMUL_DIR, "_build", "libchunks_emul.so")
TILE = 2048


@pytest.fixture(scope="module")
def emul():
    os.makedirs(os.path.dirname(EMUL_SO), exist_ok=True)
    srcs = [os.path.join(EMUL_DIR, "chunks_emul.cpp")] + [os.path.join(ROOT, "libaec_amd", "csrc", h) for h in
                                                           ("aec_chunks.h", "aec_lane.h")]
    if not os.path.exists(EMUL_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMUL_SO) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", EMUL_SO, srcs[0]],
                       check=True)
    lib = C.CDLL(EMUL_SO)
    lib.emul_chunks.restype = C.c_longlong
    return lib


def counts(samples, bs, rsi):
    blocks = (samples + bs - 1) // bs
    spr = (rsi + 63) // 64
    return blocks, (blocks // rsi) * spr + (blocks % rsi + 63) // 64, (blocks + rsi - 1) // rsi


def samples_for_segs(segs, bs, rsi, rng):
    """a sample count whose chunk has exactly `segs` segments (the last block and the last segment partly filled)"""
    if segs == 0:
        return 0
    spr = (rsi + 63) // 64
    full, rem = divmod(segs, spr)
    blocks = full * rsi + ((rem - 1) * 64 + int(rng.integers(1, 65)) if rem else 0)     # (rem * 64 < rsi)
    samples = blocks * bs - int(rng.integers(0, bs))
    assert counts(samples, bs, rsi)[1] == segs, (segs, samples, bs, rsi)
    return samples


def plain(samples, bs, rsi, spw, bits, clamp):
    """chunk after chunk, segment after segment"""
    spr = (rsi + 63) // 64
    base, cbits, start, kin, table, waves, zero_words, empty = [], [], [], [], [], [], set(), []
    s = 0
    at = 0            # bytes in front
    for i, smp in enumerate(samples):
        _, segs, rsis = counts(smp, bs, rsi)
        base.append(at * 8)
        pos, lo, hi = at * 8, 0, 31
        for j in range(segs):
            if j % spr == 0:
                table.append(pos)
            if j % spw == 0:
                waves.append(i)
                zero_words.add(pos >> 5)
            start.append(pos)
            kin.append(min(max(0, lo), hi))
            blo, bhi = int(clamp[s]) & 0xFF, int(clamp[s]) >> 8
            lo, hi = min(max(lo, blo), bhi), min(max(hi, blo), bhi)
            pos += int(bits[s])
            s += 1
        table.append(pos)
        total = pos - at * 8
        cbits.append(total)
        if segs:
            zero_words.update(((pos >> 5), (pos >> 5) + 1))
            empty.append(None)
        else:
            empty.append(at)
        at += (total + 7) // 8 if total else 1
    return base, cbits, start, kin, table, waves, zero_words, empty, at


def run(emul, rng, bs, rsi, spw, seg_counts, zero_bits_frac=0.0):
    samples = np.array([samples_for_segs(int(k), bs, rsi, rng) for k in seg_counts], dtype=np.uint64)
    n = len(samples)
    per = [counts(int(x), bs, rsi) for x in samples]
    nseg, entries = sum(p[1] for p in per), sum(p[2] + 1 for p in per)
    nwaves = sum((p[1] + spw - 1) // spw for p in per)
    bits = rng.integers(0, 70000, size=max(nseg, 1)).astype(np.uint32)
    bits[rng.random(bits.size) < zero_bits_frac] = 0
    lo = rng.integers(0, 14, size=bits.size)
    hi = lo + rng.integers(0, 14, size=bits.size) % (14 - lo)
    clamp = (lo | (hi << 8)).astype(np.uint16)
    clamp[rng.random(bits.size) < 0.4] = 31 << 8                    # segments of zero blocks leave k alone
    want = plain([int(x) for x in samples], bs, rsi, spw, bits, clamp)
    cap_words = (want[8] + 3) // 4 + 4
    base, cbits = np.zeros(n, np.uint64), np.full(n, 0xDEAD, np.uint64)
    start, kin = np.zeros(max(nseg, 1), np.uint64), np.zeros(max(nseg, 1), np.uint8)
    table, waves = np.full(entries, 0xDEAD, np.uint64), np.full(max(nwaves, 1), 0xDEAD, np.uint32)
    zeroed, empty, total = np.zeros(cap_words, np.uint8), np.zeros(n, np.uint64), np.zeros(1, np.uint64)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    got = emul.emul_chunks(C.c_uint32(bs), C.c_uint32(rsi), C.c_uint32(spw), vp(samples), C.c_uint64(n), vp(bits), vp(clamp),
                           C.c_uint64(nseg), vp(base), vp(cbits), vp(start), vp(kin), vp(table), C.c_uint64(entries), vp(waves),
                           C.c_uint64(nwaves), vp(zeroed), C.c_uint64(cap_words), vp(empty), vp(total))
    assert got == nseg
    w_base, w_bits, w_start, w_kin, w_table, w_waves, w_zero, w_empty, w_total = want
    assert base.tolist() == w_base
    assert cbits.tolist() == w_bits
    assert start[:nseg].tolist() == w_start
    assert kin[:nseg].tolist() == w_kin
    assert table.tolist() == w_table
    assert waves[:nwaves].tolist() == w_waves
    assert int(total[0]) == w_total
    assert set(np.flatnonzero(zeroed).tolist()) == {w for w in w_zero if w < cap_words}
    assert [None if e == 0xFFFFFFFFFFFFFFFF else int(e) for e in empty] == w_empty
    return nseg


@pytest.mark.parametrize("bs,rsi,spw", [(8, 128, 1), (16, 64, 2), (32, 100, 4), (8, 1, 8), (24, 5, 1), (8, 4096, 8)])
def test_chunk_borders_around_tile_borders(emul, bs, rsi, spw):
    rng = np.random.default_rng(bs * 100 + rsi)
    for first in (TILE - 1, TILE, TILE + 1, 1, 2 * TILE - 1, 2 * TILE + 1):
        for second in (1, TILE - 1, TILE, TILE + 1):
            run(emul, rng, bs, rsi, spw, [first, second, 3, 0, TILE + 5])


def test_chunks_spanning_three_tiles_and_more(emul):
    rng = np.random.default_rng(7)
    run(emul, rng, 8, 128, 8, [5, 3 * TILE - 7, 1, 2 * TILE + 9, 4100, 0, 2049, 2048, 6 * TILE + 1])
    run(emul, rng, 16, 17, 4, [3 * TILE, 3 * TILE, 3 * TILE + 1], zero_bits_frac=0.5)


@pytest.mark.parametrize("empties", [1, 9, 40])
def test_runs_of_empty_chunks(emul, empties):
    rng = np.random.default_rng(empties)
    for spw in (1, 2, 4, 8):
        run(emul, rng, 8, 128, spw, [0] * empties + [3] + [0] * empties + [TILE + 1] + [0] * empties)
        run(emul, rng, 8, 128, spw, [2, 1] + [0] * empties + [1, 1, 1] + [0] * empties, zero_bits_frac=0.7)
    run(emul, rng, 8, 128, 1, [0] * empties)


@pytest.mark.parametrize("n", [1, 3000])
def test_one_chunk_and_three_thousand(emul, n):
    rng = np.random.default_rng(n)
    if n == 1:
        for segs in (1, 7, TILE, TILE + 1, 4100):
            run(emul, rng, 8, 128, 8, [segs])
    else:
        segs = rng.integers(0, 12, size=n)
        segs[rng.random(n) < 0.1] = 0
        segs[17], segs[1500] = 2 * TILE + 3, TILE - 1
        total = run(emul, rng, 16, 33, 2, segs, zero_bits_frac=0.2)
        assert total > 8 * TILE
