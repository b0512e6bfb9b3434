"""aec_gpu_estimate_async on the device (include/aec_gpu.h; kernels: libaec_amd/csrc/aec_est.hip) against the oracle and
against aec_gpu_encode_plan_async: for every case, total_bits[i] is the oracle's total for candidate i, ~0 for a size not
asked for, best as defined -- and four plan calls on the same device buffer give the same numbers.  The cases are
tests/estimate_cases.py's: parameter sets x RSI vectors x lengths x data, the crafted zero runs, and one input of a few MiB
that spans several workgroups of every kernel of the call."""
import ctypes as C

import numpy as np
import pytest

import estimate_cases as ec
from helpers import AEC_CONF_ERROR, oracle_encode

pytestmark = pytest.mark.gpu

NONE = (1 << 64) - 1


class Device:
    """one context; every data set is uploaded once and all its RSI vectors are enqueued before one synchronisation"""

    def __init__(self, bps, flags):
        import torch
        from libaec_amd import gpu
        self.torch, self.gpu = torch, gpu
        self.bps, self.flags = bps, flags
        self.codec = gpu.Codec(bps, 16, ec.RSI_ALL, flags)
        lib = self.codec.lib
        lib.aec_gpu_held_bytes.restype = C.c_size_t
        lib.aec_gpu_held_bytes.argtypes = [C.c_void_p]
        lib.aec_gpu_trim.restype = None
        lib.aec_gpu_trim.argtypes = [C.c_void_p, C.c_size_t]

    def upload(self, data):
        a = np.ascontiguousarray(data, dtype=np.uint8)
        return self.torch.from_numpy(np.concatenate([a, np.zeros(16, np.uint8)])).cuda(), int(a.size)

    def run(self, data, vecs):
        """[(total_bits[4], best, pad)] per RSI vector from the estimate, and {(i, rsi): total_bits} from plan calls"""
        torch, gpu, codec = self.torch, self.gpu, self.codec
        d_in, n = self.upload(data)
        d_est = torch.full((len(vecs), gpu.ESTIMATE_DTYPE.itemsize), 0xA5, dtype=torch.uint8, device="cuda")
        cands = sorted({(i, ec.rsi_of(v, i)) for v in vecs for i in range(4) if ec.rsi_of(v, i)})
        d_plan = torch.full((len(cands), gpu.ENC_RESULT_DTYPE.itemsize), 0xA5, dtype=torch.uint8, device="cuda")
        st = codec._stream(None)
        for j, vec in enumerate(vecs):
            assert codec.estimate_async(d_in, n, vec, d_est[j]) == 0, vec
            if j == 0:          # plan calls in between: the two share the context's workspace, one call after the other
                for c, (i, r) in enumerate(cands):
                    p = gpu.Params(self.bps, 8 << i, r, self.flags)
                    rc = codec.lib.aec_gpu_encode_plan_async(codec.ctx, C.byref(p), d_in.data_ptr(), n, d_plan[c].data_ptr(), st)
                    assert rc == 0, (i, r)
        torch.cuda.synchronize()
        est = d_est.cpu().numpy().view(gpu.ESTIMATE_DTYPE).reshape(-1)
        plan = d_plan.cpu().numpy().view(gpu.ENC_RESULT_DTYPE).reshape(-1)
        return ([([int(t) for t in e["total_bits"]], int(e["best"]), int(e["pad"])) for e in est],
                {c: int(plan[k]["total_bits"]) for k, c in enumerate(cands)})

    def check(self, key, data, vecs):
        got, plans = self.run(data, vecs)
        for vec, (total, best, pad) in zip(vecs, got):
            want, want_best = ec.expected(key, data, self.bps, self.flags, vec)
            print(key, vec, total, best, flush=True)
            assert total == want and best == want_best and pad == 0, (key, vec, total, want, best, want_best)
            for i in range(4):
                r = ec.rsi_of(vec, i)
                assert total[i] == (plans[(i, r)] if r else NONE), (key, vec, i)


@pytest.fixture(scope="module")
def devices():
    made = {}

    def get(bps, flags):
        if (bps, flags) not in made:
            made[(bps, flags)] = Device(bps, flags)
        return made[(bps, flags)]
    yield get
    for d in made.values():
        d.codec.close()


@pytest.mark.parametrize("bps,flags", ec.PARAMS, ids=[ec.param_id(p) for p in ec.PARAMS])
def test_matrix(devices, bps, flags):
    """every length x every kind of data x every RSI vector"""
    dev = devices(bps, flags)
    rng = np.random.default_rng(1000 + bps * 64 + flags)
    for kind in ec.KINDS:
        for n in ec.LENGTHS:
            dev.check((kind, n), ec.make_data(rng, kind, n, bps, flags), ec.RSI_VECTORS)


@pytest.mark.parametrize("bps,flags", ec.PARAMS, ids=[ec.param_id(p) for p in ec.PARAMS])
def test_crafted_zero_runs(devices, bps, flags):
    """runs of 4, 5, 64 and 65 blocks of 8 at 0, 8 and 24 samples behind an RSI start: other runs for every size"""
    dev = devices(bps, flags)
    rng = np.random.default_rng(7 + bps)
    for vi, vec in enumerate(ec.RSI_VECTORS):
        dev.check(("crafted", vi), ec.crafted_zero_runs(rng, bps, flags, vec), [vec])


@pytest.mark.parametrize("bps,flags,mib", [(8, ec.PP, 2), (16, ec.PP | ec.MSB, 3), (32, ec.PP, 4), (24, ec.PP | ec.B3, 3)],
                         ids=["n8", "n16msb", "n32", "n24b3"])
def test_a_few_mib(devices, bps, flags, mib):
    """several workgroups of k_est_blocks (128 pieces each), more segments than one workgroup of k_est_sum takes in one
    round, several atomic partial sums per size; the input ends inside a piece"""
    rng = np.random.default_rng(bps)
    n = (mib << 20) // ec.bytes_per_sample(bps, flags) + 37
    lo, hi = ec.value_range(bps, flags)
    step = np.rint(rng.standard_normal(n) * rng.choice([0.3, 2, 40, 3000], size=n, p=[0.4, 0.4, 0.15, 0.05])).astype(np.int64)
    step[rng.integers(0, n, size=40)[:, None] + np.arange(3000)[None, :] - 3000] = 0        # constant stretches
    v = np.clip((lo + hi) // 2 + np.cumsum(step), lo, hi)
    data = ec.pack_samples(v, bps, flags)
    devices(bps, flags).check(("mib", bps), data, [[128] * 4, [3, 5, 7, 2], [4096, 0, 0, 65]])


def test_conf_errors(devices):
    import torch
    from libaec_amd import gpu
    dev = devices(8, ec.PP)
    codec = dev.codec
    d_in, n = dev.upload(np.arange(4096, dtype=np.uint8))
    d_est = torch.zeros(40, dtype=torch.uint8, device="cuda")
    st = codec._stream(None)

    def call(p, rsi, d_in_ptr=d_in.data_ptr(), est=d_est.data_ptr(), ctx=None, nbytes=n):
        return codec.lib.aec_gpu_estimate_async(codec.ctx if ctx is None else ctx, C.byref(p) if p else None, d_in_ptr, nbytes,
                                                gpu._rsi4(rsi), est, st)
    ok = gpu.Params(8, 16, 17, ec.PP)
    assert call(ok, None) == 0
    for bps, flags in [(0, ec.PP), (33, ec.PP), (1, ec.PP | ec.SIGNED), (6, ec.PP | ec.RESTRICTED)]:
        assert call(gpu.Params(bps, 16, 17, flags), None) == AEC_CONF_ERROR, (bps, flags)
    assert call(ok, [128, 128, 128, 4097]) == AEC_CONF_ERROR
    assert call(ok, [0, 0, 0, 0]) == AEC_CONF_ERROR
    assert call(gpu.Params(8, 16, 0, ec.PP), None) == AEC_CONF_ERROR
    assert call(None, None) == AEC_CONF_ERROR
    assert call(ok, None, est=None) == AEC_CONF_ERROR
    assert call(ok, None, d_in_ptr=d_in.data_ptr() + 4) == AEC_CONF_ERROR          # not 16-byte aligned
    assert call(ok, None, d_in_ptr=None) == AEC_CONF_ERROR
    assert call(ok, None, d_in_ptr=None, nbytes=0) == 0                            # nothing to read
    assert call(gpu.Params(8, 0, 17, ec.PP), None) == 0                            # block_size is ignored
    assert call(gpu.Params(8, 7, 17, ec.PP), [0, 0, 9, 0]) == 0
    torch.cuda.synchronize()


def test_enqueue_only_same_bytes_and_held_memory():
    """a context of its own: nothing held before, the same record twice, nothing held after a trim to 0"""
    import torch
    from libaec_amd import gpu
    dev = Device(16, ec.PP)
    codec = dev.codec
    rng = np.random.default_rng(3)
    data = ec.make_data(rng, "walk", 70000, 16, ec.PP)
    d_in, n = dev.upload(data)
    assert codec.lib.aec_gpu_held_bytes(codec.ctx) == 0
    d_a = torch.full((40,), 0x11, dtype=torch.uint8, device="cuda")
    d_b = torch.full((40,), 0xEE, dtype=torch.uint8, device="cuda")
    vec = [128, 64, 32, 16]
    assert codec.estimate_async(d_in, n, vec, d_a) == 0
    held = codec.lib.aec_gpu_held_bytes(codec.ctx)
    plan = gpu.estimate_plan(16, ec.PP, vec, n)
    assert held == plan["workspace_bytes"] > 0
    assert codec.estimate_async(d_in, n, vec, d_b) == 0                 # finds room: nothing grows, nothing synchronises
    assert codec.lib.aec_gpu_held_bytes(codec.ctx) == held
    torch.cuda.synchronize()
    assert d_a.cpu().numpy().tobytes() == d_b.cpu().numpy().tobytes()
    rec = d_a.cpu().numpy().view(gpu.ESTIMATE_DTYPE)[0]
    want, want_best = ec.expected(("held", 0), data, 16, ec.PP, vec)
    assert [int(t) for t in rec["total_bits"]] == want and int(rec["best"]) == want_best
    assert codec.estimate(d_in[:n], vec) == (want, want_best)
    codec.lib.aec_gpu_trim(codec.ctx, 0)
    assert codec.lib.aec_gpu_held_bytes(codec.ctx) == 0
    codec.close()


@pytest.mark.parametrize("bps,bs,rsi,flags", [(16, 16, 128, ec.PP), (8, 8, 64, ec.PP), (32, 32, 4096, ec.PP)])
def test_an_encode_behind_an_estimate_is_the_oracles(bps, bs, rsi, flags):
    import torch
    from libaec_amd import gpu
    rng = np.random.default_rng(bps)
    data = ec.make_data(rng, "walk", 50000, bps, flags)
    rc, want, _, offs, bits = oracle_encode(data, bps, bs, rsi, flags)
    codec = gpu.Codec(bps, bs, rsi, flags)
    d_in = torch.from_numpy(np.ascontiguousarray(data)).cuda()
    d_est = torch.zeros(40, dtype=torch.uint8, device="cuda")
    for vec in (None, [4096] * 4):
        assert codec.estimate_async(d_in, d_in.numel(), vec, d_est) == 0
        d_out, nbytes, tb, _, d_off = codec.encode(d_in)
        assert tb == bits and d_out[:nbytes].cpu().numpy().tobytes() == want
        assert np.array_equal(d_off.cpu().numpy()[:-1].astype(np.uint64), offs)
    i = {8: 0, 16: 1, 32: 2, 64: 3}[bs]
    assert codec.estimate(d_in, [rsi if j == i else 0 for j in range(4)])[0][i] == bits
    codec.close()
