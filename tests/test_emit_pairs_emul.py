"""The small-block emitter on sample pairs (libaec_amd/csrc/aec_lane.h: pairs_eligible, emit_small_pairs) on the CPU:
tests/emul/emit_pairs_emul.cpp emits every block twice into zeroed images, with emit_block and with the new emitter, and
compares the images word for word (1), checks that no bit outside the block's own is touched and that a lane which is not
eligible touches none (2), that the directed cases land on the side of the eligibility test they were built for (3) and
that the random sweeps meet both sides (4).

The sweep: block sizes 8 and 16; id_len 3 (8-bit samples) and 4 (16-bit); split with k = 0 .. kmax, second extension and
zero-run codes; with and without the reference sample; every lead 0 .. 31, in four different words.  A combination is
(block size, id_len, option and k, reference): 100 000 seeded-random blocks each, the lead moving with the block, so that
a lead sees 3 125 blocks of each combination.  Directed, at every lead: unary regions of exactly 63, 64 and 65 bits (never
eligible: the header shares their 64 bits), header + unary region of exactly 63, 64 and 65 bits, field regions of exactly
64 bits and the next k, zero-run codes that end at bit 64 and 65, and 128-bit values that start and end on word borders.
Exhaustive: every block of 8 residuals out of {0, 1, 2, 3}."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
EMUL_SO = os.path.join(EMUL_DIR, "_build", "libemit_pairs_emul.so")
SRCS = [os.path.join(EMUL_DIR, "emit_pairs_emul.cpp"), os.path.join(ROOT, "libaec_amd", "csrc", "aec_lane.h")]


@pytest.fixture(scope="module")
def emul():
    os.makedirs(os.path.dirname(EMUL_SO), exist_ok=True)
    if not os.path.exists(EMUL_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMUL_SO) for s in SRCS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", EMUL_SO, SRCS[0]], check=True)
    lib = C.CDLL(EMUL_SO)
    lib.emul_emit_pairs.restype = C.c_int
    lib.emul_emit_pairs_exhaustive.restype = C.c_int
    return lib


@pytest.mark.parametrize("seed", [1, 2])
def test_sweep_and_directed(emul, seed):
    out = (C.c_uint64 * 3)()
    rc = emul.emul_emit_pairs(C.c_uint64(100000), C.c_uint64(seed), out)
    blocks, eligible, refused = (int(x) for x in out)
    assert rc == 0, (rc, blocks)
    # 2 block sizes x (6 + 2 and 14 + 2 options) x 2 x 100 000, and the directed cases
    assert blocks > 2 * 24 * 2 * 100000 and eligible > blocks // 4 and refused > blocks // 4


def test_exhaustive_blocks_of_8(emul):
    out = (C.c_uint64 * 3)()
    rc = emul.emul_emit_pairs_exhaustive(out)
    assert rc == 0, (rc, int(out[0]))
    assert int(out[0]) == 65536 * 2 * (7 + 15)        # every block, with and without reference, every k and SE, both id_len


def test_sanitized_program(tmp_path):
    """the same program with its own main under AddressSanitizer and UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "emit_pairs_emul_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wno-unknown-pragmas", "-DEMIT_PAIRS_EMUL_MAIN", "-o", exe, SRCS[0]], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "emit_pairs_emul ok" in out.stdout, (out.stdout[-1000:], out.stderr[-3000:])
