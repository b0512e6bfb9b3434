"""The encoder route that codes every block once (libaec_amd/csrc/aec_enc_local.h) on the CPU: tests/emul/enc_local_emul.cpp
runs the header's functions -- the guess, the test for a miss, the slot geometry, the word arithmetic of the placement --
on blocks that are a length, an own clamp or none, and bits that depend on the k the block is coded with.  It checks itself
(a non-zero return names the property): the test for a miss fires for a run if and only if a block of it got another k than
the true carry gives (20: false positive, 21: false negative); the placed stream is the blocks' bits with their true k, bit
for bit (40), zero up to the padding word (41); a word taken by atomic OR is one the scan zeroes (31) and every other word
of the stream has exactly one writer (32, 33, 34); a run fits its slot (10)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
EMUL_SO = os.path.join(EMUL_DIR, "_build", "libenc_local_emul.so")
SRCS = [os.path.join(EMUL_DIR, "enc_local_emul.cpp")] + [os.path.join(ROOT, "libaec_amd", "csrc", h) for h in
                                                         ("aec_enc_local.h", "aec_lane.h")]
RULE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def emul():
    os.makedirs(os.path.dirname(EMUL_SO), exist_ok=True)
    if not os.path.exists(EMUL_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMUL_SO) for s in SRCS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", EMUL_SO, SRCS[0]], check=True)
    lib = C.CDLL(EMUL_SO)
    lib.emul_enc_local.restype = C.c_int
    return lib


def run(lib, seg_blocks, lens, lo, hi, spw, k_in=0, guess=RULE, start_bit=0, slot_words=None):
    """seg_blocks: blocks per segment.  Returns (runs that missed, runs, words taken by atomic OR)."""
    blk0 = np.concatenate([[0], np.cumsum(seg_blocks)]).astype(np.uint64)
    lens, lo, hi = (np.ascontiguousarray(lens, dtype=np.uint32), np.ascontiguousarray(lo, dtype=np.uint8),
                    np.ascontiguousarray(hi, dtype=np.uint8))
    if slot_words is None:
        per_seg = max(int(lens[int(blk0[s]):int(blk0[s + 1])].sum()) for s in range(len(seg_blocks)))
        slot_words = (spw * per_seg + 31) // 32 + 1
    out = (C.c_uint64 * 3)()
    rc = lib.emul_enc_local(C.c_uint64(len(seg_blocks)), blk0.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p),
                            lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p), C.c_uint32(spw), C.c_uint32(k_in),
                            C.c_uint32(guess), C.c_uint32(start_bit), C.c_uint32(slot_words), out)
    assert rc == 0, rc
    return int(out[0]), int(out[1]), int(out[2])


def random_blocks(rng, nseg, max_blocks, max_len, wide=0.3, none=0.3):
    seg_blocks = rng.integers(1, max_blocks + 1, nseg)
    n = int(seg_blocks.sum())
    lo = rng.integers(0, 14, n)
    hi = lo + np.where(rng.random(n) < wide, rng.integers(1, 5, n), 0)
    skip = rng.random(n) < none                      # zero blocks and continuations: no k
    lens = np.where(skip & (rng.random(n) < 0.5), 0, rng.integers(1, max_len + 1, n))
    first = np.concatenate([[0], np.cumsum(seg_blocks)[:-1]])
    lens[first] = np.maximum(lens[first], 1)         # a segment's first block always emits
    return seg_blocks, lens, np.where(skip, 255, lo), np.where(skip, 0, hi)


@pytest.mark.parametrize("spw", [1, 2, 4, 8])
def test_random_runs(emul, spw):
    rng = np.random.default_rng(100 + spw)
    missed = runs = 0
    for it in range(60):
        nseg = int(rng.integers(1, 90))
        args = random_blocks(rng, nseg, 64 if it % 4 == 0 else 5, int(rng.choice([3, 40, 300])))
        guess = RULE if it % 3 else int(rng.integers(0, 40))
        m, r, _ = run(emul, *args, spw, k_in=int(rng.integers(0, 14)), guess=guess, start_bit=int(rng.integers(0, 8)))
        missed, runs = missed + m, runs + r
    assert 0 < missed < runs                         # both outcomes of the test for a miss were seen


@pytest.mark.parametrize("spw", [1, 2, 4, 8])
def test_many_runs_in_one_word(emul, spw):
    """segments of one block of one to three bits: with one segment per run ten and more runs share a 32-bit word"""
    rng = np.random.default_rng(7 + spw)
    nseg = 200
    lens = rng.integers(1, 4, nseg)
    lo = rng.integers(0, 6, nseg)
    _, runs, ored = run(emul, np.ones(nseg, dtype=np.int64), lens, lo, lo + rng.integers(0, 3, nseg), spw,
                        start_bit=int(rng.integers(0, 8)))
    assert runs == (nseg + spw - 1) // spw and ored >= 1


@pytest.mark.parametrize("spw", [1, 8])
@pytest.mark.parametrize("lead", [0, 31])
def test_lead_and_word_borders(emul, spw, lead):
    """the second run starts at bit `lead` of a word; the stream ends on a word border; the last run is empty"""
    rng = np.random.default_rng(lead + spw)
    nseg = 3 * spw
    lens = rng.integers(1, 60, nseg)
    lens[spw - 1] += (lead - int(lens[:spw].sum())) % 32                     # first run: lead bits beyond a word border
    lens[-1] += (-int(lens.sum())) % 32                                      # the stream ends on a border
    lo = rng.integers(0, 6, nseg)
    run(emul, np.ones(nseg, dtype=np.int64), lens, lo, lo + 2, spw)
    # ... and an empty run behind it
    more = np.concatenate([lens, np.zeros(spw, dtype=np.int64)])
    lo2 = np.concatenate([lo, np.full(spw, 255)])
    run(emul, np.ones(nseg + spw, dtype=np.int64), more, lo2, np.where(lo2 == 255, 0, lo2 + 2), spw)


def test_miss_behind_the_first_segment(emul):
    """Runs of 8 segments whose first segment is zero blocks only (an odd number of bits, no k) and whose second segment
    starts with a plateau [2, 6] behind a carried k of 9 or 0: the guess (2) misses in every other run, in segment 1, at a
    bit that is on no word border; the block behind it has a plateau of one k, so segments 2 .. 7 are not coded again and
    the range's last word goes on with bits that stay (local_redo_head / local_redo_tail)."""
    spw, runs = 8, 9
    seg_blocks, lens, lo, hi = [], [], [], []
    for r in range(runs):
        for sgm in range(spw):
            seg_blocks.append(3)
            if sgm == 0:
                lens += [7, 0, 0]; lo += [255, 255, 255]; hi += [0, 0, 0]
            elif sgm == 1:
                lens += [13, 21, 9]; lo += [2, 5, 5]; hi += [6, 5, 5]
            elif sgm == spw - 1:
                lens += [11, 5, 3]; lo += [5, 5, 9 if r % 2 == 0 else 0]; hi += [5, 5, 9 if r % 2 == 0 else 0]
            else:
                lens += [17, 4, 6]; lo += [5, 5, 5]; hi += [5, 5, 5]
    missed, n, _ = run(emul, seg_blocks, lens, lo, hi, spw, start_bit=3)
    assert n == runs and missed == 4                 # the runs behind a carried 9: 1, 3, 5, 7


@pytest.mark.parametrize("bps,bs,id_len", [(16, 16, 4), (8, 16, 3), (16, 8, 4), (8, 8, 3), (8, 32, 3), (2, 8, 1)])
@pytest.mark.parametrize("rsi", [128, 64, 17, 1])
def test_slot_geometry(emul, bps, bs, id_len, rsi):
    """A segment -- 64 blocks, or the rsi blocks of a shorter RSI -- in the longest option there is (uncompressed, whose
    reference sample is its first sample: id_len + bs * bps bits) fits its share of the slot.  The share is the bound the
    kernels' LDS image has had all along (id_len + bs * bps + 2 + bps a block), so what it leaves over is (2 + bps) bits a
    block and not a bit more; a slot is its runs' shares rounded up to 128 bytes."""
    nb = min(64, rsi)
    for spw in (1, 2, 4, 8):
        out = (C.c_uint32 * 2)()
        emul.emul_local_geometry(C.c_uint32(id_len), C.c_uint32(bs), C.c_uint32(bps), C.c_uint32(rsi), C.c_uint32(spw), out)
        share, slot_words = int(out[0]), int(out[1])
        worst = nb * (id_len + bs * bps)
        assert worst <= share and share - worst == nb * (2 + bps)
        assert slot_words % 32 == 0 and spw * share <= slot_words * 32 < spw * share + 32 * 32
    # a run of segments that fill their shares through the emulator: it fits (code 10 otherwise); with 1024 bits more
    # (more than the rounding to 128 bytes can leave) it does not
    lens = np.full(nb * 8, share // nb)
    lo = np.full(nb * 8, 3)
    run(emul, np.full(8, nb), lens, lo, lo, 8, slot_words=slot_words)
    lens[0] += 1024
    with pytest.raises(AssertionError):
        run(emul, np.full(8, nb), lens, lo, lo, 8, slot_words=slot_words)


def miss_rates(emul, kind, bps, bs, mib=16, spw=8, rsi=128):
    """the count on the bench generator's data (libaec_amd/csrc/datagen.c; kind 0: C2's, kind 2: C5's), shard 0"""
    gen = C.CDLL(os.path.join(ROOT, "libaec_amd", "lib", "libaec_datagen.so"))
    a = np.empty(mib << 20, dtype=np.uint8)
    gen.aec_gen_fill_parallel(C.c_uint(kind), C.c_uint64(0), C.c_void_p(a.ctypes.data), C.c_size_t(a.size // (2 if bps > 8 else 1)),
                              C.c_uint(4))
    out = (C.c_uint64 * 7)()
    emul.emul_miss_rates.restype = C.c_int
    rc = emul.emul_miss_rates(a.ctypes.data_as(C.c_void_p), C.c_uint64(a.size), C.c_uint32(bps), C.c_uint32(bs), C.c_uint32(rsi),
                              C.c_uint32(spw), out)
    assert rc == 0
    return dict(zip(("runs", "wide_first", "miss_lo", "miss_hi", "miss_mid", "k_blocks", "wide_blocks"), (int(x) for x in out)))


@pytest.mark.parametrize("kind,bps,bs", [(0, 16, 16), (2, 8, 8)])
def test_miss_rate_per_guess_rule(emul, kind, bps, bs):
    """On the generators' data a guess can miss only where the first plateau is wider than one k, and the rule the kernels
    use (lo) misses no more often than the other two (figures: profiles/r11/miss_rates.txt, written by running this file)."""
    r = miss_rates(emul, kind, bps, bs, mib=4)
    assert r["runs"] > 0 and max(r["miss_lo"], r["miss_hi"], r["miss_mid"]) <= r["wide_first"] <= r["runs"]
    assert r["miss_lo"] <= min(r["miss_hi"], r["miss_mid"]) + r["runs"] // 100


def test_sanitized_program(tmp_path):
    """the emulator with its own main under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own"""
    exe = str(tmp_path / "enc_local_emul_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wno-unknown-pragmas", "-DENC_LOCAL_EMUL_MAIN", "-o", exe, SRCS[0]], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "enc_local_emul ok" in out.stdout, (out.stdout[-1000:], out.stderr[-3000:])


if __name__ == "__main__":
    lib = emul.__wrapped__()
    for name, kind, bps, bs in (("c2", 0, 16, 16), ("c5", 2, 8, 8)):
        for spw in (8, 1):
            r = miss_rates(lib, kind, bps, bs, mib=64, spw=spw)
            n = r["runs"]
            print(f"{name} 64 MiB, {spw} segments per run: runs {n}, first plateau wide {100 * r['wide_first'] / n:.2f} %, "
                  f"miss lo {100 * r['miss_lo'] / n:.2f} %, hi {100 * r['miss_hi'] / n:.2f} %, mid {100 * r['miss_mid'] / n:.2f} %; "
                  f"blocks that update k {r['k_blocks']}, plateau wide {100 * r['wide_blocks'] / max(1, r['k_blocks']):.2f} %")
