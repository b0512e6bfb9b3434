"""The item table of aec_gpu_decode_chunks_async (libaec_amd/csrc/aec_dchunks.h) on the CPU: tests/emul/dchunks_emul.cpp runs
the functions k_dchunks_setup and the CHUNKS variants of the decode kernels call -- the chunk that owns an item, and the item's
RSI within the chunk, table entry, block count and place in the output -- and a plain loop over the chunks must give the same.
The output ranges of a chunk's items must tile its room exactly, and no two rooms overlap.  The same lists go through the
emulation once more as a program of its own built with the host sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
EMUL_SO = os.path.join(EMUL_DIR, "_build", "libdchunks_emul.so")
SRC = os.path.join(EMUL_DIR, "dchunks_emul.cpp")
HDRS = [os.path.join(ROOT, "libaec_amd", "csrc", h) for h in ("aec_dchunks.h", "aec_lane.h")]

# (bytes per sample, block size, rsi): the containers and block sizes of tests/test_gpu_encode_chunks.py's PARAM_SETS
GEOMS = [(1, 8, 128), (2, 16, 64), (2, 16, 128), (4, 32, 100), (3, 64, 17), (2, 24, 5), (2, 8, 1), (1, 8, 1)]


@pytest.fixture(scope="module")
def emul():
    os.makedirs(os.path.dirname(EMUL_SO), exist_ok=True)
    if not os.path.exists(EMUL_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMUL_SO) for s in [SRC] + HDRS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", EMUL_SO, SRC], check=True)
    lib = C.CDLL(EMUL_SO)
    lib.emul_dchunks.restype = C.c_longlong
    return lib


def counts(size, nb, bs, rsi):
    blocks = (size // nb + bs - 1) // bs
    return blocks, (blocks + rsi - 1) // rsi


def edge_sizes(nb, bs, rsi):
    blk, rsi_b = bs * nb, bs * nb * rsi
    return [0, nb - 1 if nb > 1 else 0, nb, (bs - 1) * nb, 64 * blk, 65 * blk, rsi_b, rsi_b + nb, 3 * rsi_b + 7 * nb, 0, 0,
            5 * rsi_b, rsi_b - blk, 2 * rsi_b]


def lists(nb, bs, rsi):
    rng = np.random.default_rng(nb * 1000 + bs * 10 + rsi)
    edge = edge_sizes(nb, bs, rsi)
    yield edge
    yield edge[::-1]
    yield [0, 0, 0]
    for n in (1, 2, 37, 600, 3000):
        big = 4 * rsi * bs * nb
        yield [0 if rng.random() < 0.1 else int(rng.integers(0, big)) for _ in range(n)]


def rooms(sizes, nb, bs, rsi, rng):
    """shuffled 16-byte aligned rooms of the chunks' whole blocks, gaps of 0 to 48 bytes"""
    n = len(sizes)
    off, at = np.zeros(n, dtype=np.uint64), 16 * int(rng.integers(0, 3))
    for i in rng.permutation(n):
        off[i] = at
        at += (counts(sizes[i], nb, bs, rsi)[0] * bs * nb + 15) // 16 * 16 + 16 * int(rng.integers(0, 4))
    return off


def plain(sizes, off, nb, bs, rsi, whole=None, tail=None):
    """chunk after chunk, RSI after RSI: (chunk, rin, entry, blocks, position) per item"""
    items, entry = [], 0
    for i, size in enumerate(sizes):
        blocks, rsis = counts(size, nb, bs, rsi)
        for r in range(rsis):
            room = min(rsi, blocks - r * rsi)
            if whole is None:
                found = room
            else:
                found = rsi if r < whole[i] else (min(int(tail[i]), rsi) if r == whole[i] else 0)
            items.append((i, r, entry + r, min(room, found), int(off[i]) + r * rsi * bs * nb))
        entry += rsis + 1
    return items


def run(emul, sizes, off, nb, bs, rsi, whole=None, tail=None):
    n = len(sizes)
    ob = np.array(sizes, dtype=np.uint64)
    items = sum(counts(s, nb, bs, rsi)[1] for s in sizes)
    m = max(items, 1)
    ic, inb = np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint32)
    rin, ent, pos = (np.zeros(m, dtype=np.uint64) for _ in range(3))
    aw, at = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64)
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None      # noqa: E731
    w = np.array(whole, dtype=np.uint64) if whole is not None else None
    t = np.array(tail, dtype=np.uint64) if tail is not None else None
    got = emul.emul_dchunks(nb, bs, rsi, p(ob), p(off), C.c_uint64(n), p(w), p(t), C.c_uint64(items), p(ic), p(rin), p(ent), p(inb),
                            p(pos), p(aw), p(at))
    assert got == items
    table = list(zip(ic[:items].tolist(), rin[:items].tolist(), ent[:items].tolist(), inb[:items].tolist(), pos[:items].tolist()))
    return table, aw[:n].tolist(), at[:n].tolist()


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "-".join(str(x) for x in g))
def test_every_item_is_what_a_plain_loop_gives_and_the_items_tile_the_rooms(emul, geom):
    nb, bs, rsi = geom
    rng = np.random.default_rng(sum(geom))
    for sizes in lists(nb, bs, rsi):
        off = rooms(sizes, nb, bs, rsi, rng)
        table, aw, at = run(emul, sizes, off, nb, bs, rsi)
        assert table == plain(sizes, off, nb, bs, rsi)
        # the record made of what a chunk announces: whole RSIs and the blocks of a short last one
        for i, size in enumerate(sizes):
            blocks = counts(size, nb, bs, rsi)[0]
            assert (aw[i], at[i]) == (blocks // rsi, blocks % rsi)
        # the items of a chunk lie one behind the other from the start of its room to the end of its whole blocks ...
        end = {i: int(off[i]) for i in range(len(sizes))}
        for chunk, _, _, blocks, pos in table:
            assert pos == end[chunk] and blocks > 0
            end[chunk] = pos + blocks * bs * nb
        spans = sorted((int(off[i]), end[i]) for i in range(len(sizes)))
        for i, size in enumerate(sizes):
            assert end[i] - int(off[i]) == counts(size, nb, bs, rsi)[0] * bs * nb
        # ... and no room reaches into the next
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "-".join(str(x) for x in g))
def test_a_record_never_makes_an_item_leave_its_room(emul, geom):
    """records of an index pass: streams shorter than announced decode what they hold, streams that pretend to hold more
    decode what the chunk announces"""
    nb, bs, rsi = geom
    rng = np.random.default_rng(sum(geom) + 1)
    sizes = list(lists(nb, bs, rsi))[6]                       # 600 chunks
    off = rooms(sizes, nb, bs, rsi, rng)
    whole = [int(rng.integers(0, 7)) for _ in sizes]
    tail = [int(rng.integers(0, rsi + 3)) for _ in sizes]
    table, _, _ = run(emul, sizes, off, nb, bs, rsi, whole, tail)
    assert table == plain(sizes, off, nb, bs, rsi, whole, tail)
    for chunk, r, _, blocks, pos in table:
        room_end = int(off[chunk]) + counts(sizes[chunk], nb, bs, rsi)[0] * bs * nb
        assert pos + blocks * bs * nb <= room_end


def test_the_same_lists_under_the_host_sanitizers(tmp_path):
    exe = tmp_path / "dchunks_emul_san"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wno-unknown-pragmas", "-DDCHUNKS_EMUL_MAIN", "-o", str(exe), SRC], check=True)
    want, text = [], []
    for nb, bs, rsi in GEOMS:
        rng = np.random.default_rng(nb + bs + rsi)
        for sizes in lists(nb, bs, rsi):
            off = rooms(sizes, nb, bs, rsi, rng)
            text.append(f"{nb} {bs} {rsi} {len(sizes)}")
            text += [f"{s} {int(o)}" for s, o in zip(sizes, off)]
            want.append(sum(counts(s, nb, bs, rsi)[1] for s in sizes))
    lists_file = tmp_path / "lists.txt"
    lists_file.write_text("\n".join(text) + "\n")
    r = subprocess.run([str(exe), str(lists_file)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    assert [int(line.split()[1]) for line in r.stdout.splitlines()] == want
