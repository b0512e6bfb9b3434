"""bench.py's own contract: --steps sets the timed steps, a plain run's line carries the headline fields and nothing
that takes work of its own, --full adds the rest, and --dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_caps_and_fixed_sample(tmp_path, monkeypatch):
    """Arrays beyond their cap are sampled at the same sorted positions on every call; bytes go out as float32,
    tables as float64 (unsigned 32-bit fields stay unsigned); the caps keep a dump under 64 MB."""
    import torch
    from libaec_amd import gpu
    assert sum(cap * (4 if k in ("stream", "decoded") else 8 * (2 if k == "segment_table" else 1))
               for k, cap in bench.DUMP_CAP.items()) < 64e6
    monkeypatch.setattr(bench, "DUMP_CAP", {"stream": 1000, "decoded": 5000, "rsi_offsets": 100, "segment_table": 10})
    stream = (torch.arange(3000) % 256).to(torch.uint8)
    offsets = torch.arange(500, dtype=torch.int64) * (1 << 40)
    seg = np.zeros(40, dtype=gpu.SEG_ENTRY_DTYPE)
    seg["bit"], seg["prev"] = np.arange(40) * 7, 0xFFFFFFF0
    er = np.zeros(1, gpu.ENC_RESULT_DTYPE)
    er["total_bits"], er["k_hi"] = 12345, 7
    kw = dict(stream=stream, decoded=stream[:2000], rsi_offsets=offsets, decode_result=None,
              segment_table=torch.from_numpy(seg.view(np.uint8).copy()),
              encode_result=torch.from_numpy(er.view(np.uint8).copy()))
    bench.dump_outputs(str(tmp_path / "a"), **kw)
    bench.dump_outputs(str(tmp_path / "b"), **kw)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["decoded.npy", "encode_result.npy", "rsi_offsets.npy", "segment_table.npy", "stream.npy"]
    for n in names:
        assert np.array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)), n
    d = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    pos = bench.dump_positions(3000, 1000)
    assert 0 < pos.size <= 1000 and np.all(np.diff(pos) > 0) and pos[-1] < 3000
    assert d["stream"].dtype == np.float32 and np.array_equal(d["stream"], (pos % 256).astype(np.float32))
    assert np.array_equal(d["decoded"], (np.arange(2000) % 256).astype(np.float32))         # under its cap: whole
    assert d["rsi_offsets"].dtype == np.float64
    assert np.array_equal(d["rsi_offsets"], bench.dump_positions(500, 100) * float(1 << 40))
    sp = bench.dump_positions(40, 10)
    assert d["segment_table"].shape == (sp.size, 2)
    assert np.array_equal(d["segment_table"][:, 0], sp * 7.0) and np.all(d["segment_table"][:, 1] == 0xFFFFFFF0)
    assert d["encode_result"].tolist() == [12345, 0, 0, 0, 7]


def _bench(*args, timeout=600):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], cwd=ROOT,
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_bench_plain_run_and_dump(tmp_path):
    """A plain run: the headline fields, --steps timed steps, no CPU reference or per-kernel figures; the dump holds
    the last step's stream and decoded bytes, which are the input at the sampled positions."""
    size_mib = 64
    out = _bench("--steps", "3", "--warmup", "1", "--size-mib", str(size_mib), "--dump-outputs", str(tmp_path))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0
    assert abs(out["value"] - (size_mib << 20) / (out["ms_per_step"] * 1e-3) / 1e9) < 0.01 * out["value"]
    assert not {"cpu_baseline", "roofline", "phases_ms", "decode_bare", "abi_end_to_end"} & set(out)
    nbytes, cbytes = size_mib << 20, out["config"]["compressed_bytes_rank0"]
    d = {n[:-4]: np.load(tmp_path / n) for n in os.listdir(tmp_path)}
    assert sum(os.path.getsize(tmp_path / n) for n in os.listdir(tmp_path)) < 64e6
    assert d["decoded"].dtype == np.float32 and d["stream"].dtype == np.float32
    want = bench.generate(0, nbytes, 0, 4)                              # rank 0's input (seed 0x5EED0000)
    assert np.array_equal(d["decoded"], want[bench.dump_positions(nbytes, bench.DUMP_CAP["decoded"])])
    assert d["stream"].size == bench.dump_positions(cbytes, bench.DUMP_CAP["stream"]).size
    offs = d["rsi_offsets"]
    assert offs[0] == 0 and offs[-1] == d["encode_result"][0] and np.all(np.diff(offs) > 0)
    assert (int(d["encode_result"][0]) + 7) // 8 == cbytes
    assert d["decode_result"][3] == 0                                   # status
    assert d["segment_table"].ndim == 2 and d["segment_table"][0, 0] == 0


@pytest.mark.gpu
def test_bench_full_run():
    """--full keeps what a plain run leaves out: CPU reference (the GPU stream compared with it byte for byte),
    roofline and per-kernel times, and the extras."""
    out = _bench("--full", "--steps", "2", "--warmup", "1", "--size-mib", "64")
    assert out["steps"] == 2 and out["ms_per_step"] > 0
    assert out["cpu_baseline"]["value"] > 0
    assert out["config"]["bit_exact_vs_cpu"]["compared_bytes"] == out["config"]["compressed_bytes_rank0"]
    assert out["roofline"]["kernel_ms"] > 0 and set(out["phases_ms"]) == {"analyze", "scan", "clear", "pack", "decode"}
    assert out["decode_bare"]["GBps"] > 0 and out["abi_end_to_end"]["decode_GBps"] > 0
