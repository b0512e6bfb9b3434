"""The libaec 1.1 offsets API (RSI offset tables, aec_buffer_seek, aec_decode_range) is declared and exported: no GPU
needed -- the built library, the header and the Python mirror."""
import ctypes as C
import os
import re
import subprocess

import pytest

from helpers import ROOT

NAMES = ("aec_encode_enable_offsets", "aec_encode_count_offsets", "aec_encode_get_offsets", "aec_buffer_seek",
         "aec_decode_enable_offsets", "aec_decode_count_offsets", "aec_decode_get_offsets", "aec_decode_range")
LIB = os.path.join(ROOT, "libaec_amd", "lib", "libaec.so.0")
HEADER = os.path.join(ROOT, "include", "libaec.h")


def _built():
    if not os.path.exists(LIB):
        pytest.skip("libaec.so.0 not built")


def test_library_exports_the_offsets_api():
    _built()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    missing = [n for n in NAMES if n not in exported]
    assert not missing, missing


def test_library_symbols_resolve_through_ctypes():
    _built()
    lib = C.CDLL(LIB)
    for n in NAMES:
        assert hasattr(lib, n), n


def test_header_declares_the_offsets_api():
    text = open(HEADER).read()
    for n in NAMES:
        assert re.search(r"LIBAEC_API\s+int\s+" + n + r"\s*\(", text), n


def test_rsi_offsets_error_code():
    text = open(HEADER).read()
    m = re.search(r"#define\s+AEC_RSI_OFFSETS_ERROR\s+\((-?\d+)\)", text)
    assert m and int(m.group(1)) == -5
    import ast
    src = open(os.path.join(ROOT, "libaec_amd", "api.py")).read()
    consts = {t.id: n.value.value if isinstance(n.value, ast.Constant) else -n.value.operand.value
              for n in ast.parse(src).body if isinstance(n, ast.Assign)
              for t in n.targets if isinstance(t, ast.Name) and t.id.startswith("AEC_")
              and isinstance(n.value, (ast.Constant, ast.UnaryOp))}
    assert consts.get("AEC_RSI_OFFSETS_ERROR") == -5


def test_python_mirror_names():
    src = open(os.path.join(ROOT, "libaec_amd", "api.py")).read()
    for n in ("def encode_with_offsets", "def decode_range", "def enable_offsets", "def offsets", "def buffer_seek"):
        assert n in src, n
