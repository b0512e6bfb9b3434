#!/usr/bin/env python3
"""bench.py -- encode+decode throughput of the MI355X adaptive entropy coder.

One "step" = one pass of the hot path over the rank's resident input: encode the whole shard
(analyze -> scan -> clear -> pack) and decode it again from the encoder's segment table
(start bit + preceding sample per 64 blocks; one decoder lane per segment).
Workload = BASELINE.json configs[1] shape: 4 GiB of synthetic low-entropy 16-bit samples per
GPU, block 16, rsi 128, AEC_DATA_PREPROCESS (generator: libaec_amd/csrc/datagen.c, seed
0x5EED0000 + rank).  Inputs are resident in HBM before the timed region.

    python bench.py --gpus 1 --steps 10 --warmup 2
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

`python bench.py --gpus N` with N > 1 and no WORLD_SIZE in the environment starts the N ranks ITSELF
(`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ...` as a child
process, before this process has touched HIP), passes rank 0's JSON line through and exits with the child's
code; under torchrun (WORLD_SIZE set) it is one rank of that world.

With N > 1 the ranks code ONE stream (weak scaling: 8 GiB per rank, BASELINE configuration 4 = 64 GiB over
8 ranks; 4 GiB on one GPU): every rank plans its shard,
the 24-byte plan records are all-gathered as they lie in HBM, each rank derives its start bit and
carried k on the device and emits its shard at the global bit offset, and ONE RCCL all-gather per step
plus a stitch kernel reassemble the byte-exact stream on every rank, on a side stream that overlaps
the decode of the local shard (libaec_amd/shard.py: DeviceShard).  No host round trip inside a step.

Rank 0 prints one JSON line: metric/value (whole-job GB/s of input bytes through encode+decode) and
ms_per_step.  A plain run does only what that figure needs: set up, one untimed encode + decode (the
compressed size the timed decodes read, and a round-trip check), warm up, time --steps steps.

With --full the line also carries what takes work of its own: `roofline` for the dominant kernel
(HIP-event time per kernel over the timed steps; traffic from the committed PMC summary of exactly
this configuration, else null), `cpu_baseline` (the reference libaec -- or the oracle port if
oracle/_ref is absent -- on one host core over the WHOLE input, whose stream the GPU's is compared with
byte for byte) and, unless --no-extras: `cpu_baseline_all_cores`, `decode_bare` (index pass + decode of
the stream alone, no encoder side information), `abi_end_to_end` (pinned); with N > 1 also `comm` and
the checks of the sharded path (see below).

--dump-outputs DIR writes, after the timed steps, what the last timed step computed as DIR/<name>.npy
(float32 / float64, under 64 MB in all): `stream` (compressed bytes), `decoded` (decoded bytes),
`rsi_offsets` (the encoder's RSI start bits), `segment_table` (start bit, preceding sample per segment),
`encode_result` and `decode_result`.  An array longer than its cap is a seeded sample of fixed positions
(the same on every run with the same arguments), as are the inputs, so that two builds can be compared.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)

BPS, BS, RSI = 16, 16, 128
FLAGS = 8               # AEC_DATA_PREPROCESS
KIND = 0                # datagen.c: 0 lowent16, 1 lowent32s, 2 chunks8

# BASELINE.json configs; the headline metric is quoted on c2 (default)
CONFIGS = {
    "c2": ("lowent16", 0, 16, 16, 128, 8),               # 16-bit LSB unsigned, block 16, rsi 128, PP
    "c3": ("lowent32s", 1, 32, 32, 4096, 8 | 4 | 1),      # 32-bit signed MSB, block 32, rsi 4096, PP
    "c5": ("chunks8", 2, 8, 8, 128, 8),                   # 8-bit, block 8, rsi 128, PP (SZIP chunk shape)
    # BASELINE.json configs[0]: the reference's own sample (data/typical.rz decoded, 1 MiB of real
    # 16-bit MSB data, ratio 1.42) tiled to the workload size; -n16 -j64 -r256 -m
    "typical": ("typical.dat tiled", -1, 16, 64, 256, 8 | 4),
}


def generate(kind, nbytes, shard, threads):
    lib = C.CDLL(os.path.join(ROOT, "libaec_amd", "lib", "libaec_datagen.so"))
    a = np.empty(nbytes, dtype=np.uint8)
    lib.aec_gen_fill_parallel(C.c_uint(kind), C.c_uint64(shard), C.c_void_p(a.ctypes.data),
                              C.c_size_t(nbytes // {0: 2, 1: 4, 2: 1}[kind]), C.c_uint(threads))
    return a


def generate_to_device(kind, nbytes, shard, d_in, piece, keep=0):
    """The generator's walk in pieces (its state carries over: libaec_amd/csrc/datagen.c aec_gen_state), every piece
    uploaded at once.  Returns the first `keep` bytes on the host (an empty array for keep == 0)."""
    import torch
    lib = C.CDLL(os.path.join(ROOT, "libaec_amd", "lib", "libaec_datagen.so"))
    st = (C.c_uint64 * 5)()                               # aec_gen_state: s, x, i, hold | kind
    lib.aec_gen_init(st, C.c_uint(kind), C.c_uint64(shard))
    bps = {0: 2, 1: 4, 2: 1}[kind]
    kept = np.empty(min(keep, nbytes), dtype=np.uint8)
    buf = np.empty(piece, dtype=np.uint8)
    for o in range(0, nbytes, piece):
        n = min(piece, nbytes - o)
        lib.aec_gen_fill(st, C.c_void_p(buf.ctypes.data), C.c_size_t(n // bps))
        d_in[o:o + n].copy_(torch.from_numpy(buf[:n]))
        if o < kept.size:
            kept[o:min(o + n, kept.size)] = buf[:min(n, kept.size - o)]
    return kept


def typical_tiled(nbytes):
    """The non-synthetic point: tests/golden/typical.rz (the reference's data/typical.rz) decoded
    by the product library and repeated to `nbytes` (1 MiB = 32 whole RSIs, so tiles stay aligned)."""
    from libaec_amd import api
    rz = open(os.path.join(ROOT, "tests", "golden", "typical.rz"), "rb").read()
    rc, dec = api.aec_buffer_decode(rz, 16, 64, 256, 8 | 4, 1 << 20)
    assert rc == 0 and len(dec) == 1 << 20
    one = np.frombuffer(dec, dtype=np.uint8)
    return np.tile(one, (nbytes + one.size - 1) // one.size)[:nbytes].copy()


def measured_traffic(kernel, size_mib, config):
    """HBM bytes per launch of `kernel` from the newest committed rocprofv3 PMC summary taken on THIS
    configuration and workload size (profiles/*/traffic_*.json, written by tests/prof_traffic.sh:
    FETCH_SIZE and WRITE_SIZE in separate passes, gfx950 FETCH correction applied where the access is
    wide).  None when there is no summary for exactly this configuration -- never another one's."""
    import glob
    best = None
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*", "traffic_*.json"))):
        try:
            d = json.load(open(f))
        except (OSError, ValueError):
            continue
        if d.get("size_mib") == size_mib and d.get("config", "c2") == config and kernel in d.get("kernels", {}):
            best = (d["kernels"][kernel]["traffic"], os.path.relpath(f, ROOT))
    return best


def cpu_baseline(sample):
    """Reference libaec (oracle/_ref) if it travelled with the repo, else the oracle port;
    one thread, in memory, encode + decode of `sample`."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers
    kind = "reference" if helpers.have_ref() else "port"
    t0 = time.perf_counter()
    if kind == "reference":
        rc, enc = helpers.ref_encode(sample, BPS, BS, RSI, FLAGS)
    else:
        rc, enc, *_ = helpers.oracle_encode(sample, BPS, BS, RSI, FLAGS)
    t1 = time.perf_counter()
    if kind == "reference":
        rc2, dec = helpers.ref_decode(enc, BPS, BS, RSI, FLAGS, sample.size)
    else:
        rc2, dec, _ = helpers.oracle_decode(enc, BPS, BS, RSI, FLAGS, sample.size)
    t2 = time.perf_counter()
    assert rc == 0 and rc2 == 0 and dec == sample.tobytes()
    n = sample.size
    return {"value": round(n / (t2 - t0) / 1e9, 4), "unit": "GB/s", "cores": 1, "kind": kind,
            "sample": f"first {n >> 20} MiB of the rank-0 input, aec_buffer_encode + aec_buffer_decode "
                      f"in memory, 1 thread",
            "encode_GBps": round(n / (t1 - t0) / 1e9, 4), "decode_GBps": round(n / (t2 - t1) / 1e9, 4),
            "compressed_bytes": len(enc)}, enc


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def host_cores():
    """Host cores this process may really use: its affinity, capped by a container's CPU quota."""
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            cores = max(1, min(cores, -(-int(quota) // int(period))))
    except (OSError, ValueError):
        pass
    return cores


def cpu_all_cores(host, seconds=3.0):
    """The reference on every host core: the input cut into contiguous RSI-aligned shards, one
    independent stream per core (the reference has no threading),
    driven by the pthread harness oracle/mt_harness.c; passes are repeated to about `seconds`."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers
    mt_so = os.path.join(ROOT, "oracle", "_build", "libaec_mt.so")
    if not helpers.have_ref() or not os.path.exists(mt_so):
        return None
    cores = host_cores()
    rsi_bytes = RSI * BS * ((BPS + 7) // 8)
    per = min(64 << 20, host.size // cores) // rsi_bytes * rsi_bytes
    if per == 0:
        return None
    ref, mt = helpers.ref_lib(), C.CDLL(mt_so)
    mt.aec_mt_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_uint,
                              C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_double)]
    enc = C.cast(ref.aec_buffer_encode, C.c_void_p)
    dec = C.cast(ref.aec_buffer_decode, C.c_void_p)
    dt = C.c_double(0)

    def run(reps):
        rc = mt.aec_mt_run(enc, dec, host.ctypes.data, per, cores, reps, BPS, BS, RSI, FLAGS, C.byref(dt))
        assert rc == 0, "multi-thread reference run failed"
        return dt.value

    t1 = run(1)                            # calibrate, then repeat to about `seconds`
    reps = max(1, min(1000, int(seconds / max(t1, 1e-3))))
    if reps > 1:
        run(reps)
    return {"value": round(cores * per * reps / dt.value / 1e9, 3), "unit": "GB/s", "cores": cores,
            "cpu": cpu_model(), "kind": "reference",
            "sample": f"{cores} independent streams of {per >> 20} MiB (contiguous RSI-aligned shards of the "
                      f"rank-0 input), one pthread each, {reps} encode+decode passes in memory"}


def abi_end_to_end(host_sample):
    """PCIe-inclusive rate of the drop-in ABI: aec_buffer_encode / aec_buffer_decode of the product
    library on PINNED host buffers: H2D, kernels, D2H; the decode also finds the RSI starts first,
    because a bare stream carries no entry points.  Reported beside `value`, never as `value`."""
    import torch
    from libaec_amd import api
    lib = api.library()
    n = host_sample.size
    t_host = torch.from_numpy(host_sample).pin_memory()
    host = t_host.numpy()
    t_enc = torch.zeros(n + n // 8 + (1 << 20), dtype=torch.uint8).pin_memory()      # (room for incompressible data)
    t_dec = torch.zeros(n, dtype=torch.uint8).pin_memory()
    enc, dec = t_enc.numpy(), t_dec.numpy()

    def call(fn, src, src_len, dst):
        st = api.AecStream()
        st.next_in, st.avail_in = src.ctypes.data, src_len
        st.next_out, st.avail_out = dst.ctypes.data, dst.size
        st.bits_per_sample, st.block_size, st.rsi, st.flags = BPS, BS, RSI, FLAGS
        t0 = time.perf_counter()
        rc = getattr(lib, fn)(C.byref(st))
        return rc, st.total_out, time.perf_counter() - t0

    call("aec_buffer_encode", host, 1 << 20, enc)                     # warm (module load, first launch)
    rc, clen, t_enc = call("aec_buffer_encode", host, n, enc)
    # the first decode of a process also loads the decoder's code objects and allocates the index workspace
    # (a quarter of a gigabyte): reported beside the second, which is what a caller decoding chunk after chunk sees
    rc1, _, t_cold = call("aec_buffer_decode", enc, clen, dec)
    rc2, dlen, t_dec = call("aec_buffer_decode", enc, clen, dec)
    assert rc == 0 and rc1 == 0 and rc2 == 0 and dlen == n and np.array_equal(dec, host)
    return {"sample_MiB": n >> 20, "encode_GBps": round(n / t_enc / 1e9, 3),
            "decode_GBps": round(n / t_dec / 1e9, 3), "decode_first_call_GBps": round(n / t_cold / 1e9, 3),
            "compressed_bytes": int(clen),
            "note": "one aec_buffer_encode / aec_buffer_decode call on pinned host buffers through "
                    "libaec.so.0: init, H2D, kernels (decode: + RSI index pass), D2H, end"}


# elements kept per array (an array longer than this is sampled at seeded positions): 16.8 MB of float32 each for
# the byte arrays, 16.8 MB and 8.4 MB of float64 for the tables -- at most 59 MB in all
DUMP_CAP = {"stream": 4 << 20, "decoded": 4 << 20, "rsi_offsets": 2 << 20, "segment_table": 512 << 10}


def dump_positions(n, cap):
    """The fixed sample of an output of n elements: sorted distinct positions in [0, n), at most cap of them."""
    if n <= cap:
        return np.arange(n, dtype=np.int64)
    return np.unique(np.random.default_rng(0x5EED).integers(0, n, size=cap, dtype=np.int64))


def dump_outputs(out_dir, **arrays):
    """Writes the device tensors `arrays` (name -> tensor or None) as out_dir/<name>.npy.  Bytes become float32,
    tables and result records float64 (bit offsets stay exact below 2^53)."""
    import torch
    from libaec_amd import gpu
    os.makedirs(out_dir, exist_ok=True)
    for name, t in arrays.items():
        if t is None:
            continue
        if name == "segment_table":              # SEG_ENTRY_DTYPE: (start bit, preceding sample) per segment
            t = torch.stack([t.view(torch.int64)[0::2], t.view(torch.int32)[2::4].to(torch.int64) & 0xFFFFFFFF], dim=1)
        elif name in ("encode_result", "decode_result"):
            rec = t.cpu().numpy().view(gpu.ENC_RESULT_DTYPE if name == "encode_result" else gpu.DEC_RESULT_DTYPE)[0]
            np.save(os.path.join(out_dir, name + ".npy"),
                    np.array([float(rec[f]) for f in rec.dtype.names if f != "pad"], dtype=np.float64))
            continue
        if t.shape[0] > DUMP_CAP[name]:
            t = t[torch.from_numpy(dump_positions(t.shape[0], DUMP_CAP[name])).to(t.device)]
        a = t.to(torch.float32 if t.dtype == torch.uint8 else torch.float64).cpu().numpy()
        np.save(os.path.join(out_dir, name + ".npy"), a)


def launch_ranks(n):
    """`bench.py --gpus N` outside torchrun: start the N ranks as a CHILD process (one rank per GPU, rendezvous on
    127.0.0.1) and hand its output and exit code on.  Nothing in this process has touched HIP at this point, and it
    never does: replacing a process that has initialised the GPU is not allowed on the pool, a child is."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.run(cmd, env=env).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10, help="timed steps (at least 1)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline figure does not need: CPU reference and the "
                         "byte-for-byte comparison with its stream, the extras (see --no-extras), per-kernel times "
                         "and roofline, and with N > 1 the checks of the sharded path and the `comm` record")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last one computed (rank 0's) to DIR/<name>.npy")
    ap.add_argument("--size-mib", type=int, default=0,
                    help="input bytes per GPU (MiB); default 4096 on one GPU (BASELINE config 2), 8192 per rank with "
                         "several (config 4: 64 GiB over 8 ranks)")
    ap.add_argument("--cpu-sample-mib", type=int, default=0,
                    help="prefix of the input the one-core CPU reference codes (0 = the whole input, "
                         "1 GiB for the slow 8-bit configuration); the GPU stream is compared with all of it")
    ap.add_argument("--config", choices=sorted(CONFIGS), default="c2",
                    help="BASELINE.json configuration (the headline metric is quoted on c2)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true",
                    help="skip the untimed extras of the line: reference on all host cores, bare-stream "
                         "decode (index pass + lane-per-RSI decode, no encoder side information), "
                         "PCIe-inclusive ABI rate")
    ap.add_argument("--extras", action="store_true", help="(kept for old command lines: extras are on by default)")
    ap.add_argument("--share-gpu", action="store_true",
                    help="test mode: all ranks on cuda:0, exchange over gloo through the host (the whole N > 1 path on "
                         "a box with one GPU; NOT a scaling measurement)")
    ap.add_argument("--no-gather", action="store_true",
                    help="N > 1: independent shard streams, no exchange and no all-gather")
    ap.add_argument("--overlap", action="store_true",
                    help="pipeline steps over two HIP streams (encode of step i+1 beside decode of step i)")
    ap.add_argument("--shard-path", action="store_true",
                    help="run the plan/exchange/emit/gather/stitch path even with one GPU")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args.gpus))
    global BPS, BS, RSI, FLAGS, KIND
    wl_name, KIND, BPS, BS, RSI, FLAGS = CONFIGS[args.config]

    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    assert torch.cuda.is_available(), "bench.py needs a HIP device (the codec has no CPU path)"
    if args.share_gpu:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        if args.share_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)

    from libaec_amd import gpu

    if not args.size_mib:
        args.size_mib = 4096 if world == 1 else 8192
    nbytes = args.size_mib << 20
    threads = max(1, host_cores() // max(1, world))
    codec = gpu.Codec(BPS, BS, RSI, FLAGS)
    codec.reserve(nbytes)
    d_in = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    step = 256 << 20
    if KIND >= 0 and nbytes > (4096 << 20):
        # shards beyond 4 GiB: the same walk (seed 0x5EED0000 + rank), produced piece by piece so that the host
        # never holds more than one piece per rank; rank 0 keeps a 4 GiB prefix for the CPU reference
        host = generate_to_device(KIND, nbytes, rank, d_in, step, keep=(4096 << 20) if rank == 0 else 0)
    else:
        host = typical_tiled(nbytes) if KIND < 0 else generate(KIND, nbytes, rank, threads)
        for o in range(0, nbytes, step):
            d_in[o:o + step].copy_(torch.from_numpy(host[o:o + step]))
    n_rsi, n_blk = codec.rsi_count(nbytes), codec.block_count(nbytes)
    d_out = torch.empty(codec.encode_bound(nbytes), dtype=torch.uint8, device=dev)
    d_off = torch.empty(n_rsi + 1, dtype=torch.int64, device=dev)
    d_eres = torch.zeros(gpu.ENC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_dres = torch.zeros(40, dtype=torch.uint8, device=dev)
    d_dec = torch.empty(nbytes + 16, dtype=torch.uint8, device=dev)
    # the encoder also leaves its segment table (start bit + preceding sample per 64 blocks), which
    # lets the decoder run one lane per segment instead of one per RSI
    n_seg = codec.segment_count(nbytes)
    d_seg = torch.zeros(n_seg * 16, dtype=torch.uint8, device=dev)
    codec.set_segment_table(d_seg)

    # (AEC_BENCH_NOCHECK=enc: differential-profile builds of the ENCODER write garbage streams; they are
    # timed without the decode)
    enc_only = os.environ.get("AEC_BENCH_NOCHECK") == "enc"

    def decode_async(in_bytes):
        if not enc_only:
            codec.decode_segments_async(d_out, in_bytes, d_seg, n_seg, n_blk, d_dec, d_dres)

    # ---- untimed: one encode to learn the compressed size, correctness of the timed configuration
    codec.encode_async(d_in, nbytes, d_out, d_off, d_eres)
    eres = d_eres.cpu().numpy().view(gpu.ENC_RESULT_DTYPE)[0]
    assert not eres["overflow"]
    cbytes = (int(eres["total_bits"]) + 7) // 8
    decode_async(cbytes)
    dres = d_dres.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)[0]
    if not os.environ.get("AEC_BENCH_NOCHECK"):       # (differential-profile builds decode wrong on purpose)
        assert dres["status"] == 0, "decode reported an error"
        assert torch.equal(d_dec[:nbytes], d_in), "round trip differs"

    cpu, exact = None, None
    if rank == 0 and args.full and not args.no_cpu_baseline:
        # One host core codes the WHOLE input with the reference (about 15-30 s; the 8-bit configuration,
        # four times slower per byte, a 1 GiB prefix) and EVERY byte of the GPU stream is compared with
        # what it produced (a prefix of whole RSIs codes to a prefix of the stream).
        mib = args.cpu_sample_mib or (1024 if args.config == "c5" else args.size_mib)
        sample = host[: min(nbytes, host.size, mib << 20)]
        cpu, enc_cpu = cpu_baseline(sample)
        whole = sample.size == nbytes
        ncmp = len(enc_cpu) if whole else len(enc_cpu) - 1
        assert whole is False or len(enc_cpu) == cbytes, "GPU stream length != CPU reference stream length"
        ref_np = np.frombuffer(enc_cpu, dtype=np.uint8)
        for o in range(0, ncmp, 256 << 20):
            hi = min(ncmp, o + (256 << 20))
            assert np.array_equal(d_out[o:hi].cpu().numpy(), ref_np[o:hi]), "GPU stream != CPU reference stream"
        exact = {"compared_bytes": ncmp, "of_stream_bytes": cbytes, "input_MiB": sample.size >> 20}
        del ref_np, enc_cpu
    extras = {}
    if rank == 0 and args.full and not args.no_extras:
        extras["cpu_baseline_all_cores"] = cpu_all_cores(host)
        # ---- bare stream: no offset table, no segment table -- what a stream from another producer
        # looks like.  Index pass (speculative tables + walk) + lane-per-RSI decode, timed together.
        d_idx = torch.zeros(n_rsi + 2, dtype=torch.int64, device=dev)
        d_ires = torch.zeros(40, dtype=torch.uint8, device=dev)
        # (long RSIs: the index pass also leaves the segment starts and the decoder takes a lane per segment, the
        # sample in front of each from a summing pass -- include/aec_gpu.h: aec_gpu_index_segments_async)
        d_sbits = torch.zeros((n_rsi + 2) * codec.segments_per_rsi(), dtype=torch.int64, device=dev)
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        t_idx, t_dec = [], []
        for _ in range(3):
            d_idx.zero_()
            d_dec.zero_()
            e0.record()
            codec.index_segments_async(d_out, cbytes, 0, d_idx, d_sbits, n_rsi + 1, d_ires)
            e1.record()
            codec.decode_bare_async(d_out, cbytes, d_idx, d_sbits, n_rsi, n_blk, None, d_dec, d_dres)
            e2.record()
            torch.cuda.synchronize()
            t_idx.append(e0.elapsed_time(e1))
            t_dec.append(e1.elapsed_time(e2))
        ires = d_ires.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)[0]
        assert int(ires["n_rsi"]) == n_rsi and torch.equal(d_idx[:n_rsi], d_off[:n_rsi]), "index pass != encoder's table"
        assert torch.equal(d_dec[:nbytes], d_in), "bare-stream round trip differs"
        ti, td = sorted(t_idx)[1], sorted(t_dec)[1]
        extras["decode_bare"] = {"GBps": round(nbytes / ((ti + td) * 1e-3) / 1e9, 2), "index_ms": round(ti, 3),
                                 "decode_ms": round(td, 3),
                                 "note": "aec_gpu_index_segments_async + aec_gpu_decode_bare_async (a lane per RSI; per "
                                         "segment where RSIs hold eight segments and more) on the stream alone, median of 3"}
        del d_idx, d_sbits
        extras["abi_end_to_end"] = abi_end_to_end(host[: 256 << 20])
    del host

    if args.full:
        # achievable HBM rate beside the spec peak: a plain device copy of the same input (N read + N written)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        d_dec[:nbytes].copy_(d_in)
        ev0.record()
        for _ in range(3):
            d_dec[:nbytes].copy_(d_in)
        ev1.record()
        torch.cuda.synchronize()
        copy_gbps = 2 * nbytes * 3 / (ev0.elapsed_time(ev1) * 1e-3) / 1e9

    # ---- N > 1: ONE stream over all ranks (libaec_amd/shard.py): plan -> exchange 3 numbers ->
    # emit at the global bit offset -> one RCCL all-gather of the slices -> local stitch.  The
    # all-gather + stitch run on a side stream and overlap the decode of the local shard.
    from libaec_amd import shard
    sharded = (world > 1 and not args.no_gather) or args.shard_path
    if sharded:
        # sizes for the all-gather come from one untimed plan (the timed steps never go to the host)
        codec.encode_plan_async(d_in, nbytes, d_eres)
        r0 = d_eres.cpu().numpy().view(gpu.ENC_RESULT_DTYPE)[0]
        if world > 1:
            plans0 = shard.exchange_plans(int(r0["total_bits"]), int(r0["k_lo"]), int(r0["k_hi"]),
                                          device="cpu" if args.share_gpu else dev)
        else:
            plans0 = [(int(r0["total_bits"]), int(r0["k_lo"]), int(r0["k_hi"]))]
        slot = shard.slot_bytes(plans0)
        assert slot <= d_out.numel()
        dsh = shard.DeviceShard(codec, rank, world, slot)
        d_stream = torch.zeros(sum((b + 7) // 8 for b, _, _ in plans0) + 64, dtype=torch.uint8, device=dev)
        d_total = torch.zeros(1, dtype=torch.int64, device=dev)
        my_start = sum(b for b, _, _ in plans0[:rank])
        mine = (my_start % 8 + plans0[rank][0] + 7) // 8
        comm = torch.cuda.Stream(device=dev)

    # Two HIP streams: the encode of step i+1 runs beside the decode of step i (double-buffered
    # compressed stream and segment table), which fills the bubbles each kernel leaves on its own.
    overlap = args.overlap and not sharded
    if overlap:
        s_enc, s_dec = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
        outs = [d_out, torch.empty_like(d_out)]
        segs = [d_seg, torch.zeros_like(d_seg)]
        enc_done = [torch.cuda.Event(), torch.cuda.Event()]
        dec_done = [torch.cuda.Event(), torch.cuda.Event()]
        step_no = [0]
        for e in dec_done:
            e.record()

    def one_step():
        if overlap:
            i = step_no[0] & 1
            step_no[0] += 1
            with torch.cuda.stream(s_enc):
                s_enc.wait_event(dec_done[i])                 # buffer i is free again
                codec.set_segment_table(segs[i])
                codec.encode_async(d_in, nbytes, outs[i], d_off, d_eres)
                enc_done[i].record()
            with torch.cuda.stream(s_dec):
                s_dec.wait_event(enc_done[i])
                codec.decode_segments_async(outs[i], cbytes, segs[i], n_seg, n_blk, d_dec, d_dres)
                dec_done[i].record()
            return
        if not sharded:
            codec.encode_async(d_in, nbytes, d_out, d_off, d_eres)
            decode_async(cbytes)
            return
        # plan -> 24-byte all-gather of the plan records as they lie in HBM -> emit at the global bit
        # offset (start bit and carried k derived on the device) -> [side stream: all-gather of the
        # slices + stitch kernel] beside the decode of the local shard.  No host round trip.
        dsh.step(d_in, nbytes, d_out, d_off, d_eres)
        ready = torch.cuda.Event()
        ready.record()
        with torch.cuda.stream(comm):
            comm.wait_event(ready)
            dsh.gather_and_stitch(d_out, d_stream, d_total)
        decode_async(mine)
        torch.cuda.current_stream().wait_stream(comm)

    if sharded and args.full:
        # correctness of the sharded configuration before timing it: local round trip, and on one
        # rank the stitched stream must be exactly the single-device stream
        one_step()
        torch.cuda.synchronize()
        assert torch.equal(d_dec[:nbytes], d_in), "sharded round trip differs"
        # ... and the shard decoded out of the STITCHED stream (what every rank holds after the all-gather): the
        # segment table of the shard, moved to where the shard lies in the whole stream
        seg64 = d_seg.view(torch.int64).view(-1, 2).clone()
        seg64[:, 0] += 8 * (my_start // 8)
        d_dec.zero_()
        codec.decode_segments_async(d_stream, d_stream.numel() - 64, seg64.view(torch.uint8).view(-1), n_seg, n_blk,
                                    d_dec, d_dres)
        dres = d_dres.cpu().numpy().view(gpu.DEC_RESULT_DTYPE)[0]
        assert dres["status"] == 0 and torch.equal(d_dec[:nbytes], d_in), "shard decoded from the stitched stream differs"
        del seg64
        if world == 1:
            ref_out = torch.empty_like(d_out)
            codec.encode_async(d_in, nbytes, ref_out, d_off, d_eres)
            assert torch.equal(ref_out[:cbytes], d_stream[:cbytes]), "stitched stream != single stream"
            del ref_out
        elif args.share_gpu and rank == 0 and KIND >= 0 and world * nbytes <= (8 << 30):
            # (test mode) the stream all ranks stitched together must be what ONE encoder makes of the inputs of
            # all ranks one behind the other (every rank's input is its seeded walk: generated again here)
            whole = torch.empty(world * nbytes, dtype=torch.uint8, device=dev)
            for r in range(world):
                h = generate(KIND, nbytes, r, threads)
                whole[r * nbytes:(r + 1) * nbytes].copy_(torch.from_numpy(h))
            c2 = gpu.Codec(BPS, BS, RSI, FLAGS)
            w_out, w_bytes, w_bits, _, _ = c2.encode(whole)
            total = int(d_total.cpu().item()) if d_total is not None else w_bytes
            assert total == w_bytes and torch.equal(w_out[:w_bytes], d_stream[:w_bytes]), \
                "stream stitched from all ranks != single-encoder stream of the concatenated inputs"
            del whole, w_out, c2

    # ---- N > 1: what a reader of the line needs to check that N ranks on N devices exchanged over the fabric
    # (VERDICT round 4, item 8): the process group's own answers, every rank's device, the size of the all-gather and a
    # checksum of the stitched stream that every rank must agree on
    comm_info = None
    if world > 1 and args.full:
        import hashlib
        props = torch.cuda.get_device_properties(dev)
        mine_dev = {"rank": rank, "device": torch.cuda.current_device(), "name": props.name,
                    "pci_bus_id": getattr(props, "pci_bus_id", None), "pci_device_id": getattr(props, "pci_device_id", None),
                    "uuid": str(getattr(props, "uuid", "")), "pid": os.getpid()}
        stitched = None
        if sharded:
            total = int(d_total.cpu().item())
            body = d_stream[: total - total % 8].view(torch.int64)
            stitched = {"bytes": total, "sum64": int(body.sum().item()) & 0xFFFFFFFFFFFFFFFF}
            if total <= (1 << 30):
                stitched["sha16"] = hashlib.sha256(d_stream[:total].cpu().numpy().tobytes()).hexdigest()[:16]
        gathered = [None] * world
        dist.all_gather_object(gathered, {"dev": mine_dev, "stitched": stitched})
        devs = [g["dev"] for g in gathered]
        ids = {(d["uuid"], d["pci_bus_id"], d["device"]) for d in devs}
        if not args.share_gpu:
            assert len(ids) == world, f"{world} ranks on {len(ids)} distinct devices: {devs}"
        if sharded:
            assert all(g["stitched"] == gathered[0]["stitched"] for g in gathered), "ranks hold different stitched streams"
        comm_info = {"backend": dist.get_backend(), "world_size": dist.get_world_size(), "devices": devs,
                     "distinct_devices": len(ids),
                     "allgather_bytes": (slot * world) if sharded else 0,
                     "plan_exchange_bytes": 24 * world if sharded else 0,
                     "stitched": gathered[0]["stitched"]}

    if args.full:
        lib = gpu._lib()
        lib.aec_gpu_profile.argtypes = [C.c_void_p, C.c_int]
        lib.aec_gpu_phase_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    for _ in range(args.warmup):
        one_step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    if args.full:
        lib.aec_gpu_profile(codec.ctx, 1)  # events only; nothing waits on them until the loop is over
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one_step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if args.share_gpu else dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    if args.dump_outputs and rank == 0:
        if overlap:
            last = (step_no[0] - 1) & 1
            stream, seg = outs[last][:cbytes], segs[last]
        elif sharded:
            stream, seg = d_stream[:int(d_total.cpu().item())], d_seg
        else:
            stream, seg = d_out[:cbytes], d_seg
        dump_outputs(args.dump_outputs, stream=stream, decoded=None if enc_only else d_dec[:nbytes],
                     rsi_offsets=d_off, segment_table=seg, encode_result=d_eres,
                     decode_result=None if enc_only else d_dres)

    if args.full:
        # ---- per-kernel device time of the timed steps (HIP events recorded by the library, on the
        # stream the kernels ran on, around every launch of the timed region; read only now)
        ms = (C.c_float * 5)()
        lib.aec_gpu_phase_ms(codec.ctx, ms)
        lib.aec_gpu_profile(codec.ctx, 0)
        phase = dict(zip(["analyze", "scan", "clear", "pack", "decode"], [float(x) for x in ms]))

    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        value = world * nbytes / (elapsed / args.steps) / 1e9
        out = {
            "metric": "encode+decode GB/s (input bytes)",
            "value": round(value, 3),
            "unit": "GB/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u32",
            "data": "synthetic",
            "config": {"workload": f"{args.config}: {wl_name} {args.size_mib} MiB per GPU, {BPS}-bit, block {BS}, rsi {RSI}, "
                                   f"flags {FLAGS}; step = encode + decode (segment table)"
                                   + ("; one stream over all ranks: plan, exchange, emit at the global bit "
                                      "offset, RCCL all-gather + stitch overlapped with decode" if sharded else "")
                                   + ("; TEST MODE: all ranks share cuda:0 and exchange over gloo through the host -- "
                                      "the N > 1 code path, not a scaling measurement" if args.share_gpu else ""),
                       "bits_per_sample": BPS, "block_size": BS, "rsi": RSI, "flags": FLAGS,
                       "input_bytes_per_gpu": nbytes, "compressed_bytes_rank0": cbytes,
                       "ratio": round(nbytes / cbytes, 3), "bit_exact_vs_cpu": exact,
                       "parallelism": (f"{world} rank(s), one bit-exact stream" if sharded
                                       else f"{world} independent shard stream(s)")},
        }
        if args.full:
            algo = {"analyze": nbytes, "pack": nbytes + cbytes, "decode": nbytes + cbytes}
            dom = max(algo, key=lambda k: phase[k])
            achieved = algo[dom] / (phase[dom] * 1e-3) / 1e9
            traffic = measured_traffic(f"k_{dom}", args.size_mib, args.config)
            enc_ms = phase["analyze"] + phase["scan"] + phase["clear"] + phase["pack"]
            out.update({
                "roofline": {"bound": "hbm", "kernel": f"k_{dom}", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS,
                             "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5),
                             "traffic": traffic[0] if traffic else None,
                             "traffic_source": traffic[1] if traffic else None,
                             "algorithmic_bytes_per_launch": algo[dom], "kernel_ms": round(phase[dom], 4),
                             "device_copy_GBps": round(copy_gbps, 1),
                             "frac_of_device_copy": round(achieved / copy_gbps, 5)},
                "cpu_baseline": cpu,
                "phases_ms": {k: round(v, 4) for k, v in phase.items()},
                "encode_GBps": round(nbytes / (enc_ms * 1e-3) / 1e9, 2),
                "decode_GBps": round(nbytes / (phase["decode"] * 1e-3) / 1e9, 2),
                "decode_note": "decode_GBps uses the encoder's segment table (side information next to the unchanged "
                               "stream); decode_bare is the rate from the stream alone",
            })
        if comm_info:
            out["comm"] = comm_info
        out.update({k: v for k, v in extras.items() if v is not None})
        if "decode_bare" in out:
            # encode + decode WITHOUT the side table (what north_star asks of a stream any producer wrote): the timed
            # encode of the step, then index pass + lane-per-RSI decode of the bare stream
            b = out["decode_bare"]
            b["encode_plus_decode_GBps"] = round(nbytes / ((enc_ms + b["index_ms"] + b["decode_ms"]) * 1e-3) / 1e9, 2)
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
