"""Headline benchmark: 64^3 cubes/s through compress_hyper + decompress_hyper (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    (N > 1: python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...)

A plain run sets up, warms up, times the K steps and prints the headline line (`value`, `ms_per_step`, `config`).
--full adds everything below that takes runs of its own: N = 1 the roofline, the other operating points, the file-level,
stream-of-clouds and large-cloud figures, the training step, the CPU baseline and the parity block; N > 1 the collectives,
strong scaling and independent clouds.  --dump-outputs DIR writes what the last timed step returned (see _dump_outputs).

Workload (`config.workload`): a seeded synthetic stand-in for BASELINE.json configs[1]
(longdress_vox10_1300, --mode=hyper --cube_size=64): synthetic.make_cloud(seed 1300, 1024^3 grid)
-> ~830 k points -> ~205 cubes of 64^3 after the reference's partition (min_num 64), weights =
the hyper/a6b3 checkpoint trained with this repository (checkpoints/hyper/a6.00b3.00; the cloud was held out of its
training set; no checkpoint / ply of the reference exists offline).
One step = one pass of the whole batch through compress_hyper (analysis, hyper encoder, hyper decoder,
CDF kernels, host range ENcoder) and decompress_hyper (host range DEcoder, hyper decoder, CDF kernels,
synthesis), cubes resident in HBM when the clock starts.  N = 1: transform.compress_hyper + decompress_hyper.  N > 1: the sharded codec (pcgcv1_amd/sharding.py) — the ranks'
batches together are ONE cloud of N x 205 cubes in contiguous blocks (weak scaling: a rank voxelised and holds only its
block): all_reduce of the z range, gathers of z-hat / per-cube records / y strings to rank 0, which codes
the single z string; then rank 0 broadcasts the strings, every rank decodes its own prefix of the z string, decodes +
synthesises + top-k classifies its block (later ranks wait longer for their z symbols and take geometrically smaller
blocks: sharding.decode_ranges) and the bit-packed occupancy masks are gathered to rank 0.  value = cubes of all ranks / max time;
`collectives` lists bytes and ms per collective of one instrumented step, `strong_scaling` the one 205-cube cloud cut
over the N ranks, `independent_clouds` N clouds of 205 cubes, one per rank, with the single-GPU codec (no collective, N z
strings: what the format's one sequential z stream per cloud costs the sharded figure).

With --full the JSON line also carries
  roofline     — the conv kernel instantiation with the largest share of GPU time, timed with hipEvents
                 on the launch stream (pcgc_net_set_profiling) in extra steps right after the timed ones;
                 achieved = 2*MACs of that layer per launch / mean launch time, peak = 157.3 TFLOP/s fp32 MFMA.
                 Launches of the analysis that skip empty tiles are listed under keys of their own with
                 the FLOPs of the computed tiles only; `traffic` comes from the committed PMC summary and is refused
                 when that summary's kernel duration does not match the live one.
  cpu_baseline — the CPU oracle (oracle/transform.py: torch-CPU conv one cube per call + C range coder,
                 kind "port": the literal reference needs TensorFlow 1.13) on a bounded sample, rank 0, N=1 only.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")      # before the first HIP call: see pcgcv1_amd/__init__.py
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL between the ranks of one node needs it on this pool (a no-op at N = 1)

NOMINAL_SCLK_MHZ = 2400
HBM_PEAK_GBPS = 8000.0                 # MI355X_MICROARCH.md
FP32_MFMA_PEAK_TFLOPS = 157.3          # MI355X_MICROARCH.md, v_mfma_f32_16x16x4_f32 / 32x32x2_f32
# BASELINE.json's metric, verbatim; `value` is its throughput half (cubes/s), the "bpp & D1-PSNR vs reference" half is
# the `parity_vs_cpu_oracle` block of the same line (no checkpoint / cloud of the reference exists offline)
METRIC = "64\u00b3 cubes/sec encode+decode (hyper/a6b3); bpp & D1-PSNR vs reference"
GFLOP_PER_CUBE = 21.5675               # encode (A+HE+HD) + decode (HD+S)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-cubes", type=int, default=24, help="cubes in the CPU-baseline sample (0 = skip)")
    ap.add_argument("--profile", default=None,
                    help="weights of the headline: 'trained' = checkpoints/hyper/a6.00b3.00 (trained with this repository's "
                         "Trainer, tools/train_ckpt.py; the default when present), or a seeded synthetic profile: sparse, mid, dense")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the second operating point and the file-level figure")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: roofline, operating points, file level, stream / large "
                         "cloud, training step, CPU baseline + parity (N = 1); collectives, strong scaling, independent clouds (N > 1)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy (float32 / float64, at most 64 MB)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def _stream_crc(stream):
    """CRC-32 of a cloud's coded bytes (y strings in cube order, then the z string): equal across process counts"""
    import zlib
    return zlib.crc32(b"".join(bytes(s_) for s_ in stream[0]) + bytes(stream[4])) & 0xFFFFFFFF


DUMP_SAMPLE = 1 << 23          # elements kept of a larger output: 32 MB of float32


def _sample(flat):
    """a fixed, seeded sample of a large flat tensor (sorted positions; the same ones for the same size), else all of it"""
    import torch
    n = int(flat.numel())
    if n <= DUMP_SAMPLE:
        return flat.cpu().numpy()
    idx = np.sort(np.random.default_rng(1300).choice(n, DUMP_SAMPLE, replace=False))
    return flat[torch.from_numpy(idx).to(flat.device)].cpu().numpy()


def _dump_outputs(d, stream, decoded):
    """--dump-outputs: what the last timed step returned to its caller (rank 0), as DIR/<name>.npy in float32 / float64.
    The stream of compress_hyper: y_strings (bytes of all cubes' strings in cube order) + y_string_lengths, y_min_vs,
    y_max_vs, y_shape, z_string, z_min_v, z_max_v, z_shape.  N = 1, decompress_hyper's logits [B,64,64,64,1]:
    logits_cube_sums (float64 sum per cube) and logits_sample (DUMP_SAMPLE seeded positions of the flattened batch).
    N > 1, the top-k masks gathered bit-packed to rank 0: occupied_voxels_per_cube and occupancy_packed (bytes; sampled
    like the logits when larger)."""
    import torch
    os.makedirs(d, exist_ok=True)
    y_strings = [bytes(s_) for s_ in stream[0]]
    arrays = {"y_strings": np.frombuffer(b"".join(y_strings), np.uint8).astype(np.float32),
              "y_string_lengths": np.array([len(s_) for s_ in y_strings], np.float64),
              "y_min_vs": np.asarray(stream[1], np.float64), "y_max_vs": np.asarray(stream[2], np.float64),
              "y_shape": np.asarray(stream[3], np.float64),
              "z_string": np.frombuffer(bytes(stream[4]), np.uint8).astype(np.float32),
              "z_min_v": np.asarray(stream[5], np.float64), "z_max_v": np.asarray(stream[6], np.float64),
              "z_shape": np.asarray(stream[7], np.float64)}
    if torch.is_tensor(decoded):
        arrays["logits_cube_sums"] = decoded.reshape(decoded.shape[0], -1).sum(dim=1, dtype=torch.float64).cpu().numpy()
        arrays["logits_sample"] = _sample(decoded.reshape(-1)).astype(np.float32)
    else:
        packed = decoded[0]
        ones = torch.tensor([bin(v).count("1") for v in range(256)], dtype=torch.float64, device=packed.device)
        arrays["occupied_voxels_per_cube"] = ones[packed.long()].sum(dim=1).cpu().numpy()
        arrays["occupancy_packed"] = _sample(packed.reshape(-1)).astype(np.float32)
    for name, a in arrays.items():
        np.save(os.path.join(d, name + ".npy"), a)


def _self_launch(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves — a child `torch.distributed.run`, before
    this process has touched the GPU — relay rank 0's JSON line (the children inherit stdout) and exit with the child's
    code, non-zero if any rank failed."""
    import subprocess
    # --standalone: torchrun hosts the c10d rendezvous itself on a port IT binds and keeps (a port probed here by bind / close
    # could be taken by another process before the ranks meet)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1",
           "--nproc-per-node", str(args.gpus), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    return subprocess.run(cmd, env=env).returncode


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(_self_launch(args))
    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("WORLD_SIZE=%d but --gpus=%d: launch one rank per GPU (or run `python bench.py --gpus N` bare: it "
                         "starts its own ranks)" % (world, args.gpus))
    # one rank per GPU over RCCL ("nccl").  PCGC_BENCH_BACKEND=gloo + several ranks on one device is only for
    # exercising the N>1 code path on a 1-GPU box.
    backend = os.environ.get("PCGC_BENCH_BACKEND", "nccl")
    n_dev = torch.cuda.device_count()                     # does not initialise the GPU
    if world > 1 and backend == "nccl" and n_dev < world:
        # RCCL needs one device per rank: fail NOW with the reason instead of hanging in the first collective until the timeout
        sys.stderr.write("bench.py: --gpus %d over RCCL needs %d visible devices, found %d (PCGC_BENCH_BACKEND=gloo runs the ranks "
                         "on shared devices)\n" % (world, world, n_dev))
        sys.exit(3)
    local_dev = local_rank % max(1, n_dev)
    torch.cuda.set_device(local_dev)
    if world > 1:
        import datetime
        tmo = datetime.timedelta(seconds=int(os.environ.get("PCGC_BENCH_TIMEOUT_S", "300")))
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_dev), timeout=tmo)
        else:
            dist.init_process_group(backend, timeout=tmo)

    from pcgcv1_amd import checkpoint, process, synthetic, transform
    from pcgcv1_amd.models import model_voxception as model

    trained_dir = os.path.join(ROOT, "checkpoints", "hyper", "a6.00b3.00")
    if args.profile is None:
        args.profile = "trained" if os.path.isdir(trained_dir) else "sparse"

    def weights_of(profile):
        if profile == "trained":
            return checkpoint.load(trained_dir)
        if profile.startswith("trained_"):                   # the other rate points trained here: trained_a2.00b3.00, ...
            return checkpoint.load(os.path.join(ROOT, "checkpoints", "hyper", profile[len("trained_"):]))
        return synthetic.make_weights(seed=1300, profile=profile)
    weights = weights_of(args.profile)
    checkpoint._CACHE["bench"] = weights
    weights_text = ("the hyper/a6b3 checkpoint trained with this repository's train_hyper step on seeded synthetic surfaces "
                    "(checkpoints/hyper/a6.00b3.00, tools/train_ckpt.py; the cloud was held out)" if args.profile == "trained"
                    else "seeded '%s' weights of the reference architecture" % args.profile)
    pts = synthetic.make_cloud(seed=1300)
    cubes, cube_positions, points_numbers = process.preprocess_points(pts, 1.0, 64, 64)
    B = int(cubes.shape[0])

    nums = points_numbers
    if world > 1:
        from pcgcv1_amd import sharding
        ops = sharding.HipOps(model, "bench")
        quiet = sharding.Exchange()

    def step_sharded(x, total, nums_local, ex):
        """one encode + decode of a `total`-cube cloud of which this rank holds block `x`"""
        stream = sharding.compress_hyper_sharded(x, ops, total=total, points_numbers=nums_local, exchange=ex)
        masks = sharding.decompress_hyper_sharded(stream[:8] if rank == 0 else None, ops,
                                                  points_numbers=stream[8] if rank == 0 else None, exchange=ex, packed=True)
        return stream, masks

    def step_local():
        """this rank's cubes through the single-process codec (no collective: safe on one rank only)"""
        out = transform.compress_hyper(cubes, model, "bench")
        xs = transform.decompress_hyper(*out, model, "bench")
        return out, xs

    def step():
        if world > 1:
            return step_sharded(cubes, world * B, nums, quiet)
        return step_local()

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    import gc
    gc.collect()
    gc.freeze()          # a full Python collection over the set-up's objects (weights, golden tables) takes about 50 ms — one
                         # whole step — and would land in the timed region at random
    barrier()
    # the clock samples only feed the roofline block (--full)
    clock = (_ClockSampler(torch.cuda.current_device())
             if rank == 0 and args.full and os.environ.get("PCGC_BENCH_CLOCK", "1") != "0" else None)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out, xs = step()
    barrier()
    dt = time.perf_counter() - t0
    clock_report = clock.stop() if clock else None
    if args.dump_outputs and rank == 0:
        _dump_outputs(args.dump_outputs, out, xs)
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    ms_per_step = 1e3 * dt / args.steps
    value = world * B * args.steps / dt

    result = {
        "metric": METRIC, "value": round(value, 3), "unit": "cubes/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "synthetic longdress_vox10-like cloud (seed 1300, 1024^3): %d points -> %d cubes of 64^3, "
                               "--mode=hyper --cube_size=64 --min_num=64, %s, "
                               "compress_hyper + decompress_hyper incl. host range coding%s"
                               % (len(pts), B, weights_text, "" if world == 1 else
                                  "; %d such blocks = one %d-cube cloud sharded over %d ranks (sharding.py: RCCL all_reduce / "
                                  "gather / broadcast), decode ends with top-k masks gathered bit-packed to rank 0"
                                  % (world, world * B, world)),
                   "cubes_per_rank": B, "host_threads": __import__("pcgcv1_amd._lib", fromlist=["x"]).host_threads(),
                   "host_pipelines": transform._PIPES},
        "path_tflops": round(value * GFLOP_PER_CUBE / 1e3, 3),
        "ranks": {"world_size": dist.get_world_size() if world > 1 else 1, "backend": (dist.get_backend() if world > 1 else None),
                  "devices_visible": torch.cuda.device_count()},
    }

    if rank == 0:
        nbytes = sum(len(s) for s in out[0]) + len(out[4])
        result["config"]["bytes_per_cube"] = round(nbytes / (world * B), 1)
        if world == 1:
            result["config"]["stream_crc32"] = _stream_crc(out)

    # ---------------------------------------------------------------- N > 1: collectives of one step, strong scaling
    if world > 1 and args.full:
        ex = sharding.Exchange(timing=True)
        step_sharded(cubes, world * B, nums, ex)
        barrier()
        if rank == 0:
            result["collectives"] = [{"name": n_, "bytes": b_, "ms": round(m_, 3)} for n_, b_, m_ in ex.log]
            result["collective_ms_per_step"] = round(sum(m_ for _, _, m_ in ex.log), 3)
        lo, hi = sharding.shard_range(B, rank, world)
        xb, nb_ = cubes[lo:hi].contiguous(), nums[lo:hi]
        step_sharded(xb, B, nb_, quiet)
        barrier()
        t0 = time.perf_counter()
        for _ in range(3):
            st_strong, _ = step_sharded(xb, B, nb_, quiet)
        barrier()
        ds = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(ds, op=dist.ReduceOp.MAX)
        if rank == 0:
            result["strong_scaling"] = {"workload": "the one %d-cube cloud cut into %d contiguous blocks" % (B, world),
                                        "value": round(B * 3 / float(ds.item()), 3), "unit": "cubes/s",
                                        "ms_per_step": round(1e3 * float(ds.item()) / 3, 3),
                                        # the same cloud through one process gives these bytes (config.stream_crc32 at N = 1)
                                        "stream_crc32": _stream_crc(st_strong)}

        # every rank its OWN cloud (a directory of frames, BASELINE configs[2]): no collective, no shared z string — next to
        # `value`, whose one big cloud pays for the format's single z stream (coded and decoded on one thread for all ranks' cubes)
        step_local()
        barrier()
        t0 = time.perf_counter()
        for _ in range(3):
            step_local()
        barrier()
        di = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(di, op=dist.ReduceOp.MAX)
        if rank == 0:
            result["independent_clouds"] = {"workload": "%d clouds of %d cubes, one per rank, each with the single-GPU codec" % (world, B),
                                            "value": round(world * B * 3 / float(di.item()), 3), "unit": "cubes/s",
                                            "ms_per_step": round(1e3 * float(di.item()) / 3, 3)}

    # ---------------------------------------------------------------- roofline (dominant conv kernel)
    if rank == 0 and args.full and not args.no_roofline:
        c = transform.get_codec(model, "bench")
        nets = {"analysis_transform": c.analysis_transform, "synthesis_transform": c.synthesis_transform,
                "hyper_encoder": c.hyper_encoder, "hyper_decoder": c.hyper_decoder}
        # per-launch durations are a property of a kernel running alone: the two host pipelines of the timed path
        # (transform._PIPES) interleave kernels of two streams, which would stretch every event pair, so the two
        # profiling steps run single-pipeline (same kernels, same launch geometry)
        pipes = transform._PIPES
        transform._PIPES = 1
        for n in nets.values():
            n.set_profiling(True)
        for _ in range(2):
            step_local()            # rank 0 alone runs this block: never the sharded step (its collectives would hang)
        torch.cuda.synchronize()
        transform._PIPES = pipes
        agg = {}
        # empty-space skipping (analysis, 64^3 stage): those launches compute only the tiles whose receptive field holds an
        # occupied voxel — their FLOPs are counted for the computed tiles only, under keys of their own, and never make the
        # `roofline` kernel look faster than the dense launches of the same kernel (the synthesis side) are
        skip_on = os.environ.get("PCGC_SKIP_EMPTY", "3") != "0" and int(cubes.shape[1]) == 64
        seg_on = skip_on and os.environ.get("PCGC_SKIP_EMPTY", "3") == "3"
        heavy = _heavy_tile_fractions(cubes, seg_on) if skip_on else None
        if heavy:
            result["config"]["empty_space_skipping"] = {"what": "analysis, 64^3 and 32^3 stages: wave tiles whose receptive field holds no occupied voxel are "
                                                                "not computed — they equal the net's response to an empty cube (bit-identical; DESIGN.md §3)"
                                                                + ("; the C = 16 blocks of the 64^3 stage work on slots of 8 planes x 2 rows x 16 voxels "
                                                                   "(csrc/vrn_seg.hip), four to a wave" if seg_on else ""),
                                                        "computed_tile_fraction_per_launch": {k: [round(v, 4) for v in vs] for k, vs in heavy.items()}}
            if os.environ.get("PCGC_SKIP_MID", "1") == "0":
                heavy["32"] = heavy["32s"] = [1.0] * 6
                heavy["64"][7] = 1.0
        for net_name, n in nets.items():
            for r in n.profile_report():
                if r["mode"] == 2:
                    macs = r["B"] * (r["Din"] ** 3) * 27 * r["cin"] * r["cout"]
                else:
                    dout = r["Din"] // (2 if r["mode"] == 1 else 1)
                    macs = r["B"] * (dout ** 3) * (r["k"] ** 3) * r["cin"] * r["cout"]
                if r["kernel"] == "ks1":        # + fused conv2_1 (1x1x1, Cin -> Cout)
                    macs += r["B"] * (r["Din"] ** 3) * r["cin"] * r["cout"]
                elif r["kernel"] == "ks2":      # + fused conv2_3 (1x1x1, Cout -> 2 Cout)
                    macs += r["B"] * (r["Din"] ** 3) * r["cout"] * 2 * r["cout"]
                elif r["kernel"] == "vrnA":     # conv1_1 (3^3 16->4) + conv2_1 (1^3 16->4)
                    macs = r["B"] * (r["Din"] ** 3) * (27 * 16 * 4 + 16 * 4)
                elif r["kernel"] == "vrnBC":    # conv1_2 (3^3 4->8) + conv2_2 (3^3 4->4) + conv2_3 (1^3 4->8)
                    macs = r["B"] * (r["Din"] ** 3) * (27 * 4 * 8 + 27 * 4 * 4 + 4 * 8)
                elif r["kernel"] in ("rowA", "rowBC", "rowB", "rowC", "segA", "segBC"):   # row kernels: C = 16 / 32 / 64 at D = 64 / 32 / 16 (q = C / 4)
                    q = {64: 4, 32: 8, 16: 16}[r["Din"]]
                    per_vox = {"rowA": 27 * 4 * q * q + 4 * q * q, "rowBC": 27 * q * 2 * q + 27 * q * q + q * 2 * q,
                               "rowB": 27 * q * 2 * q, "rowC": 27 * q * q + q * 2 * q}[r["kernel"].replace("seg", "row")]
                    macs = r["B"] * (r["Din"] ** 3) * per_vox
                skipped = (heavy is not None and net_name == "analysis_transform" and
                           ((r["Din"] == 64 and r["kernel"] in ("rowA", "rowBC", "rowin", "rowdown", "segA", "segBC", "segin")) or (r["Din"] == 32 and r["kernel"] in ("rowA", "rowBC"))))
                if skipped and r["Din"] == 64:    # launch index in the stage: conv_in 0, block i: A 1 + 2i, BC 2 + 2i (layer = 1 + 5i + which), down_1 7
                    li = 0 if r["kernel"] in ("rowin", "segin") else (7 if r["kernel"] == "rowdown" else
                                                           1 + 2 * ((r["layer"] - 1) // 5) + (1 if r["kernel"] in ("rowBC", "segBC") else 0))
                    macs *= heavy["64"][li]
                elif skipped:                     # 32^3 stage: blocks start at layer 17; the tile shape follows the launch size
                    li = 2 * ((r["layer"] - 17) // 5) + (1 if r["kernel"] == "rowBC" else 0)
                    macs *= heavy["32s" if r["B"] <= 16 else "32"][li]
                if r["kernel"] in ("vrnA", "vrnBC", "rowA", "rowBC", "rowB", "rowC", "segA", "segBC"):
                    c = {64: 16, 32: 32, 16: 64}.get(r["Din"], 16) if r["kernel"].startswith("row") else 16
                    key = {"vrnA": "vrn16_a_kernel", "vrnBC": "vrn16_bc_kernel", "rowA": "vrn%da_row_kernel" % c,
                           "rowBC": "vrn%dbc_row_kernel" % c, "rowB": "vrn%db_row_kernel" % c,
                           "rowC": "vrn%dc_row_kernel" % c, "segA": "vrn16a_seg_kernel", "segBC": "vrn16bc_seg_kernel"}[r["kernel"]] + "@D%d" % r["Din"] + (
                               " [analysis: empty slots skipped]" if r["kernel"].startswith("seg") else (" [analysis: empty tiles skipped]" if skipped else ""))
                    a_ = agg.setdefault(key, {"ms": 0.0, "n": 0, "flop": 0.0})
                    a_["ms"] += r["ms"]; a_["n"] += 1; a_["flop"] += 2.0 * macs
                    continue
                kname = {"rowin": "conv_in_row_kernel", "segin": "conv_in_seg_kernel", "rowout": "deconv_out_row_kernel", "rowup": "up_row_kernel", "rowdown": "down_row_kernel", "rowh8": "conv8_row_kernel", "rowhup": "up8_row_kernel", "rowhdown": "down8_row_kernel", "valu": "conv_valu_kernel", "direct": "conv_direct_kernel", "mfma": "tconv_mfma_kernel" if r["mode"] == 2 else "conv_mfma_kernel",
                         "ks": "conv_ks_kernel", "ks1": "conv_ks_kernel+conv2_1", "ks2": "conv_ks_kernel+conv2_3"}[r["kernel"]]
                key = "%s<Cin=%d,Cout=%d,k=%d,mode=%d>@D%d" % (kname, r["cin"], r["cout"], r["k"], r["mode"], r["Din"]) + (" [empty tiles skipped]" if skipped else "")
                a = agg.setdefault(key, {"ms": 0.0, "n": 0, "flop": 0.0})
                a["ms"] += r["ms"]
                a["n"] += 1
                a["flop"] += 2.0 * macs
                if r["kernel"] in ("rowin", "rowout", "segin"):      # 1 <-> 16 channels at 64^3: bound by HBM, not by the matrix cores
                    # (conv_in with skipping: the tiles it does not compute are not written either — virtual tiles)
                    a["bytes"] = a.get("bytes", 0.0) + 4.0 * r["B"] * (r["Din"] ** 3) * (r["cin"] + r["cout"] * (heavy["64"][0] if skipped else 1.0))
            n.set_profiling(False)
        total_ms = sum(a["ms"] for a in agg.values())
        dom_key, dom = max(agg.items(), key=lambda kv: kv[1]["ms"])
        achieved = dom["flop"] / (dom["ms"] * 1e-3) / 1e12
        # every conv kernel of the path issues its MACs on the fp32 matrix cores except the VALU / direct fallbacks
        on_mfma = not any(t in dom_key for t in ("conv_valu", "conv_direct", "vrn16_a_kernel", "vrn16_bc_kernel"))
        result["roofline"] = {"bound": "mfma", "dominant_kernel_pipe": "mfma" if on_mfma else "valu (same fp32 peak)", "achieved": round(achieved, 3), "peak": FP32_MFMA_PEAK_TFLOPS,
                              "unit": "TFLOP/s", "frac": round(achieved / FP32_MFMA_PEAK_TFLOPS, 4), "traffic": None,
                              "kernel": dom_key, "launches": dom["n"], "avg_launch_ms": round(dom["ms"] / dom["n"], 4),
                              "share_of_conv_time": round(dom["ms"] / total_ms, 3),
                              "all_conv_tflops": round(sum(a["flop"] for a in agg.values()) / (total_ms * 1e-3) / 1e12, 3),
                              "conv_ms_per_step": round(total_ms / 2, 3)}
        result["roofline"]["traffic"], result["roofline"]["traffic_source"] = _traffic_from_profiles(dom_key, dom["ms"] / dom["n"])
        # `path_tflops` prices the step at the ALGORITHMIC (dense) work; with empty-space skipping part of it is not executed.
        # The executed FLOPs of one step (per-launch MACs of the two profiled steps, skipped launches counted for their
        # computed tiles only) over the headline's own step time give the rate the matrix cores really sustain.
        flop_step = sum(a["flop"] for a in agg.values()) / 2.0
        result["path_frac"] = round(result["path_tflops"] / FP32_MFMA_PEAK_TFLOPS, 4)
        result["path_tflops_executed"] = round(flop_step / (ms_per_step * 1e-3) / 1e12, 3)
        result["path_frac_executed"] = round(result["path_tflops_executed"] / FP32_MFMA_PEAK_TFLOPS, 4)
        result["executed_fraction_of_dense_flops"] = round(flop_step / (B * GFLOP_PER_CUBE * 1e9), 4)
        if clock_report:
            # the 157.3 TFLOP/s peak is 256 CUs x 256 flop/clk at the 2.4 GHz boost clock; under this load the part
            # settles lower (hwmon freq1_input of this GPU, sampled during the timed steps)
            f = clock_report["sclk_mhz_median"] / NOMINAL_SCLK_MHZ
            result["roofline"]["clock"] = dict(clock_report, nominal_mhz=NOMINAL_SCLK_MHZ,
                                               peak_at_measured_clock=round(FP32_MFMA_PEAK_TFLOPS * f, 1),
                                               frac_at_measured_clock=round(achieved / (FP32_MFMA_PEAK_TFLOPS * f), 4),
                                               all_conv_frac_at_measured_clock=round(result["roofline"]["all_conv_tflops"] / (FP32_MFMA_PEAK_TFLOPS * f), 4))
        top = sorted(agg.items(), key=lambda kv: -kv[1]["ms"])[:int(os.environ.get("PCGC_BENCH_TOP", "8"))]
        def mem_side(k, v):
            # bytes through L2 per launch from the committed counter passes over this launch's live duration: which
            # kernels sit at the memory roofline although they issue their MACs on the matrix cores (vrn16bc: 5.7 TB/s,
            # and tools/exp/t_ablate.py takes 23 % off its time by dropping the traffic from the same instruction stream)
            if "<" in k:                                # templated generic kernels: the summary's rows are per instantiation
                return {}
            t, _ = _traffic_from_profiles(k, v["ms"] / v["n"])
            if not t:
                return {}
            gbps = t / (v["ms"] / v["n"] * 1e-3) / 1e9
            return {"hbm_GBps": round(gbps, 1), "hbm_frac": round(gbps / HBM_PEAK_GBPS, 3)}
        result["roofline"]["top_kernels"] = [
            dict({"kernel": k, "ms_per_step": round(v["ms"] / 2, 3), "tflops": round(v["flop"] / (v["ms"] * 1e-3) / 1e12, 2)},
                 **({"bound": "hbm", "algorithmic_GBps": round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1)} if "bytes" in v else {}),
                 **mem_side(k, v))
            for k, v in top]
        result["stage_seconds"] = {k: round(v, 4) for k, v in _stage_times(transform, model, cubes).items()}

    # ---------------------------------------------------------------- second operating point + file level (N = 1)
    if rank == 0 and world == 1 and args.full and not args.no_extras:
        def sym_range(o_):
            return "y-hat in [%d, %d] per cube" % (int(np.min(o_[1])), int(np.max(o_[2])))
        result["operating_points"] = [{"profile": args.profile, "headline": True, "symbols": sym_range(out), "cubes_per_s": round(value, 1),
                                       "ms_per_step": round(ms_per_step, 3), "bytes_per_cube": result["config"]["bytes_per_cube"]}]
        # the other operating points: 'trained_<rate>' are the other checkpoints trained here (what real models hand the coder
        # across the rate range); 'sparse' / 'mid' are seeded random weights (the hyperprior predicts nothing: kilobytes per
        # cube, wide CDF rows = more D2H and host coding) — stress profiles, not rate points
        others = sorted(d_ for d_ in (os.listdir(os.path.dirname(trained_dir)) if os.path.isdir(trained_dir) else [])
                        if d_ != os.path.basename(trained_dir) and os.path.isdir(os.path.join(os.path.dirname(trained_dir), d_)))
        for prof in ["trained"] + ["trained_" + d_ for d_ in others] + ["sparse", "mid"]:
            if prof == args.profile or (prof == "trained" and not os.path.isdir(trained_dir)):
                continue
            key = "bench_" + prof
            checkpoint._CACHE[key] = weights_of(prof)

            def step2():
                o = transform.compress_hyper(cubes, model, key)
                return o, transform.decompress_hyper(*o, model, key)
            n2 = 20
            for _ in range(3):
                o2, _x = step2()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n2):
                o2, _x = step2()
            torch.cuda.synchronize()
            d2 = time.perf_counter() - t0
            result["operating_points"].append({
                "profile": prof, "headline": False, "symbols": sym_range(o2),
                "cubes_per_s": round(B * n2 / d2, 1), "ms_per_step": round(1e3 * d2 / n2, 3),
                "bytes_per_cube": round((sum(len(s_) for s_ in o2[0]) + len(o2[4])) / B, 1)})
            transform._CODECS.pop((getattr(model, "__name__", str(model)), key), None)
            checkpoint._CACHE.pop(key, None)
        result["file_level"] = _file_level(pts, B)
        result["stream_of_clouds"] = _stream_block(transform, model, cubes, B)
        result["large_cloud"] = _large_block(transform, model, cubes, B)

    # ---------------------------------------------------------------- config 4: one train_hyper step (N = 1, rank 0)
    if rank == 0 and world == 1 and args.full and not args.no_extras:
        result["train"] = _train_block()

    # ---------------------------------------------------------------- CPU baseline (oracle port), rank 0, N=1
    if rank == 0 and world == 1 and args.full and args.cpu_cubes > 0:
        from oracle import transform as otransform
        from oracle import points as opoints
        from pcgcv1_amd import metrics
        from pcgcv1_amd.dataprocess import inout_points as iop
        n = min(args.cpu_cubes, B)
        sample = cubes[:n].cpu().numpy()

        def cpu_pass(x_):
            t0_ = time.perf_counter()
            o_ = otransform.compress_hyper(x_, weights)
            xr_ = otransform.decompress_hyper(*o_, weights)
            return time.perf_counter() - t0_, o_, xr_
        # the CPU path run competently: one untimed warm-up cube (the first conv call pays thread-pool and oneDNN primitive
        # set-up: 3.5 s against 0.7 s warm on 8 cores), then the thread count that is fastest for ONE-cube convolutions
        # (the reference's tf.map_fn(parallel_iterations=1) shape; torch's default = every hardware thread of a 256-CPU
        # host is far past the optimum), then the sample at that count.  The range coder is one thread, as the TF op is.
        default_threads = torch.get_num_threads()
        cpu_pass(sample[:1])
        t_default = cpu_pass(sample[:1])[0]
        sweep = {default_threads: t_default}
        for nt in (8, 16, 32, 64, 128):
            if nt <= (os.cpu_count() or 1) and nt not in sweep:
                torch.set_num_threads(nt)
                cpu_pass(sample[:1])                       # the pool resizes on the first call
                sweep[nt] = cpu_pass(sample[:1])[0]
        best = min(sweep, key=sweep.get)
        torch.set_num_threads(best)
        cpu_pass(sample[:1])
        cdt, o, x_ref = cpu_pass(sample)
        torch.set_num_threads(default_threads)
        result["cpu_baseline"] = {"value": round(n / cdt, 4), "unit": "cubes/s", "cores": best,
                                  "kind": "port", "host_cpus": os.cpu_count(),
                                  "value_at_default_threads": round(1.0 / t_default, 4), "default_threads": default_threads,
                                  "thread_sweep_s_per_cube": {str(k): round(v, 3) for k, v in sorted(sweep.items())},
                                  "range_coder_threads": 1,
                                  "sample": "first %d cubes of the same batch, oracle/transform.py compress_hyper+"
                                            "decompress_hyper (torch-CPU fp32 conv3d, one cube per call; C range coder on one "
                                            "thread), after a warm-up cube, at the fastest of the swept thread counts, %.1f s"
                                            % (n, cdt)}
        # bpp / D1-PSNR of the HIP path vs the CPU oracle on that same sample (BASELINE metric: "bpp & D1-PSNR vs reference")
        mine = transform.compress_hyper(cubes[:n], model, "bench")
        x_mine = transform.decompress_hyper(*mine, model, "bench")
        spos = iop.ordered_positions(cube_positions)[:n]           # cubes are stored in key order
        nums = points_numbers[:n]
        orig = iop.merge_points(iop.voxels2points(sample), spos, 64)
        rec_mine = iop.merge_points(iop.voxels2points(iop.select_voxels(x_mine, nums, 1.0)), spos, 64)
        rec_ref = iop.merge_points(opoints.voxels2points(opoints.select_voxels(x_ref, nums, 1.0)), spos, 64)
        npts = float(len(orig))
        bpp_mine = 8.0 * (sum(map(len, mine[0])) + len(mine[4])) / npts
        bpp_ref = 8.0 * (sum(map(len, o[0])) + len(o[4])) / npts
        d1_mine, d1_ref = metrics.d1_psnr(orig, rec_mine, 1023), metrics.d1_psnr(orig, rec_ref, 1023)
        result["parity_vs_cpu_oracle"] = {"cubes": n, "bpp": round(bpp_mine, 5), "bpp_oracle": round(bpp_ref, 5),
                                          "d1_psnr_db": round(d1_mine, 4), "d1_psnr_db_oracle": round(d1_ref, 4),
                                          "max_abs_logit_diff": float(np.abs(x_mine.cpu().numpy() - x_ref).max()),
                                          "note": ("trained checkpoint on its held-out cloud, first cubes only; the whole cloud: "
                                                   "checkpoints/hyper/report_a6.00b3.00.json" if args.profile == "trained" else
                                                   "random (untrained) weights: absolute bpp/PSNR are meaningless, the "
                                                   "HIP-vs-oracle difference is the parity figure")}
        rep_path = os.path.join(ROOT, "checkpoints", "hyper", "report_a6.00b3.00.json")
        if args.profile == "trained" and os.path.exists(rep_path):
            with open(rep_path) as f:
                rep = json.load(f)
            result["rate_distortion"] = {"bpp": rep["bpp_files"], "d1_psnr_db": rep["d1_psnr_db"], "peak": rep["peak"],
                                         "bytes_per_cube": rep["bytes_per_cube"], "actual_over_estimated_bits": rep["actual_over_estimated"],
                                         "actual_over_quantised_table_bits": rep["actual_over_quantised_tables"],
                                         "reference_recorded": rep["reference_recorded"],
                                         "source": "checkpoints/hyper/report_a6.00b3.00.json (tools/eval_ckpt.py on this cloud)"}
    if rank == 0:
        print(json.dumps(result))
    if world > 1:
        barrier()                   # the other ranks wait for rank 0's post-processing, so that every rank leaves together
        dist.destroy_process_group()


class _ClockSampler(object):
    """Reads this GPU's shader clock and socket power from sysfs (hwmon) every 100 ms on a host thread while the timed
    steps run — what the part actually clocks at under this load.  Reports None where sysfs is not readable.  (Every read is
    a query to the GPU's management controller and a wake-up of one more Python thread next to the two pipelines: at 50 ms the
    timed region measured 0.3 ms per step slower with the sampler than without, PCGC_BENCH_CLOCK=0.)"""

    def __init__(self, device):
        import glob
        import threading
        import torch
        self.freq, self.power, self.rows = None, None, []
        try:
            pr = torch.cuda.get_device_properties(device)
            addr = "%04x:%02x:%02x" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
            for d in glob.glob("/sys/class/drm/card*/device"):
                if os.path.basename(os.path.realpath(d)).lower().startswith(addr):
                    hw = glob.glob(d + "/hwmon/hwmon*")
                    if hw and os.path.exists(hw[0] + "/freq1_input"):
                        self.freq = hw[0] + "/freq1_input"
                        self.power = hw[0] + "/power1_input" if os.path.exists(hw[0] + "/power1_input") else None
        except Exception:                                      # noqa: BLE001 (a diagnostic: never fails the bench)
            self.freq = None
        self._stop = threading.Event()
        self._thread = threading.Thread(target=self._run, daemon=True)
        if self.freq:
            self._thread.start()

    @staticmethod
    def _read(path):
        try:
            with open(path) as f:
                return float(f.read())
        except (OSError, ValueError, TypeError):
            return None

    def _run(self):
        while not self._stop.wait(0.1):
            self.rows.append((self._read(self.freq), self._read(self.power) if self.power else None))

    def stop(self):
        if not self.freq:
            return None
        self._stop.set()
        self._thread.join()
        f = sorted(r[0] / 1e6 for r in self.rows if r[0])
        w = sorted(r[1] / 1e6 for r in self.rows if r[1])
        if len(f) < 2:
            return None
        rep = {"sclk_mhz_median": round(f[len(f) // 2]), "sclk_mhz_min": round(f[0]), "sclk_mhz_max": round(f[-1]), "samples": len(f)}
        if w:
            rep["socket_power_w_median"] = round(w[len(w) // 2])
        return rep


def _heavy_tile_fractions(cubes, seg=False):
    """Fraction of wave tiles each launch of the analysis has to COMPUTE on these cubes (the rest is copied from the
    empty-cube response or not written at all): the rule of csrc/vrn_row.hip: tile_order_kernel restated on the host — a
    tile is empty when the fine (64^3) window its outputs depend on holds no occupied row.
    -> {"64": conv_in, A/BC of the three C = 16 blocks, down_1;  "32": A/BC of the three C = 32 blocks for launches of more
        than 16 cubes;  "32s": the same for small launches (2 x 2 tiles)}"""
    occ = (cubes.reshape(cubes.shape[0], 64, 64, 64) != 0).any(dim=3).cpu().numpy()           # [B, d, h]
    B = occ.shape[0]
    c = np.zeros((B, 65, 65), np.int64)
    c[:, 1:, 1:] = occ.cumsum(1).cumsum(2)

    def frac(th, ld, lo, hi, step):
        G, heavy, total = 64 // step, 0, 0
        for d0 in range(0, G, ld):
            dl, dh = max(step * d0 - lo, 0), min(step * (d0 + ld - 1) + hi, 63)
            for h0 in range(0, G, th):
                hl, hh = max(step * h0 - lo, 0), min(step * (h0 + th - 1) + hi, 63)
                heavy += int(((c[:, dh + 1, hh + 1] - c[:, dl, hh + 1] - c[:, dh + 1, hl] + c[:, dl, hl]) > 0).sum())
                total += B
        return heavy / float(total)
    def frac_slots(r):
        """segment form (csrc/vrn_seg.hip: seg_order_kernel): slots of 8 planes x 2 rows x 16 voxels whose planes, rows and voxels dilated by
        r hold an occupied voxel"""
        o = (cubes.reshape(cubes.shape[0], 64, 64, 64) != 0).cpu().numpy()
        c3 = np.zeros((B, 65, 65, 65), np.int32)
        c3[:, 1:, 1:, 1:] = o.cumsum(1, dtype=np.int32).cumsum(2, dtype=np.int32).cumsum(3, dtype=np.int32)
        heavy = 0
        for d0 in range(0, 64, 8):
            a0, a1 = max(d0 - r, 0), min(d0 + 7 + r, 63) + 1
            for h0 in range(0, 64, 2):
                b0, b1 = max(h0 - r, 0), min(h0 + 1 + r, 63) + 1
                for w0 in range(0, 64, 16):
                    e0, e1 = max(w0 - r, 0), min(w0 + 15 + r, 63) + 1
                    n = (c3[:, a1, b1, e1] - c3[:, a0, b1, e1] - c3[:, a1, b0, e1] - c3[:, a1, b1, e0]
                         + c3[:, a0, b0, e1] + c3[:, a0, b1, e0] + c3[:, a1, b0, e0] - c3[:, a0, b0, e0])
                    heavy += int((n > 0).sum())
        return heavy / float(B * 1024)
    stage64 = [frac_slots(r) for r in range(1, 8)] if seg else ([frac(2, 4, 1, 1, 1)] + [frac(2, 8, r, r, 1) for r in range(2, 8)])
    return {"64": stage64 + [frac(2, 2, 7, 9, 2)],
            "32": [frac(4 if i % 2 == 0 else 2, 4 if i % 2 == 0 else 8, 9 + 2 * i, 11 + 2 * i, 2) for i in range(6)],
            "32s": [frac(2, 2, 9 + 2 * i, 11 + 2 * i, 2) for i in range(6)]}


def _git_blob_sha1(path):
    """the object id `git hash-object` gives this file: ties the figure to one committed summary"""
    import hashlib
    with open(path, "rb") as f:
        data = f.read()
    return hashlib.sha1(b"blob %d\0" % len(data) + data).hexdigest()


def _traffic_from_profiles(dom_key, live_avg_ms=None, profiles_dir=None):
    """HBM bytes per launch of a kernel from the newest committed rocprofv3 PMC summary (profiles/*pmc_per_kernel.csv:
    separate FETCH_SIZE / WRITE_SIZE passes of this same command, FETCH doubled as MI355X_MICROARCH.md prescribes for
    gfx950).  Counters cannot be read from inside the benchmark process, so this is the committed measurement, not a live
    one — made falsifiable: the record names the file, its git blob id and the kernel's Dispatches / AvgDurationNs in that
    summary, and when the summary's duration differs from this run's live per-launch time by more than 10 % (another
    kernel version, another launch size) the bytes are REFUSED (traffic None + the reason).
    -> (bytes per launch or None, record dict or None)"""
    import csv
    import glob
    name = dom_key.split("<")[0].split("@")[0].split("+")[0].split(" [")[0]
    for path in sorted(glob.glob(os.path.join(profiles_dir or os.path.join(ROOT, "profiles"), "*pmc_per_kernel.csv")), reverse=True):
        if "_train_" in os.path.basename(path):          # the training step's kernels (other template instantiations)
            continue
        cands = []
        with open(path) as f:
            for row in csv.DictReader(f):
                if name in row["Kernel"]:
                    try:
                        cands.append((float(row["AvgDurationNs"]), float(row["FETCH_x2_MB"]) + float(row["WRITE_MB"]), int(float(row["Dispatches"])), row))
                    except (ValueError, KeyError):
                        continue
        if not cands:
            continue
        # a kernel appears in two template instantiations: the synthesis' dense launches (three blocks x every chunk: the more
        # numerous row) and the analysis' launches with empty-space skipping (two chunks per launch: half as many).  Chosen by
        # that, not by the nearest duration: the two lie 10 % apart and a slow box's dense launches land in between
        skipping = "[analysis" in dom_key
        avg_ns, mb, disp, row = (min if skipping else max)(cands, key=lambda c_: c_[2])
        rec = {"file": os.path.basename(path), "git_blob": _git_blob_sha1(path), "kernel_row": row["Kernel"],
               "dispatches": disp, "avg_duration_us": round(avg_ns / 1e3, 2),
               "fetch_x2_MB": float(row["FETCH_x2_MB"]), "write_MB": float(row["WRITE_MB"])}
        if live_avg_ms is not None:
            # the duration the committed collection is checked by: the kernel's average in the plain kernel trace of the same
            # collection (<tag>_kernel_stats_pipes1.csv) where it exists — the counter passes serialise the dispatches and run
            # this kernel 8-10 % shorter than any uninstrumented run, which put an honest match at the edge of the 10 % rule
            trace = path.replace("_pmc_per_kernel.csv", "_kernel_stats_pipes1.csv")
            if os.path.exists(trace):
                with open(trace) as f:
                    for srow in csv.DictReader(f):
                        if srow.get("Name", "").startswith(row["Kernel"]):
                            try:
                                avg_ns = float(srow["AverageNs"])
                                rec["trace_file"] = os.path.basename(trace)
                                rec["trace_avg_duration_us"] = round(avg_ns / 1e3, 2)
                            except (ValueError, KeyError):
                                pass
                            break
            dev = avg_ns / 1e6 / live_avg_ms - 1.0
            rec["live_avg_us"] = round(live_avg_ms * 1e3, 2)
            rec["duration_vs_live"] = round(dev, 4)
            if abs(dev) > 0.10:
                rec["refused"] = ("the committed summary's kernel duration differs from this run's by %+.1f %% (> 10 %%): "
                                  "it does not describe the kernel that was timed" % (100 * dev))
                return None, rec
        return round(mb * 1e6), rec
    return None, None


def _train_block(n=15):
    """BASELINE configs[3] per GPU: one train_hyper step (forward, explicit reverse pass, TF1 Adam) on a batch of 8 cubes of
    64^3, the median of n synchronised steps.  Work = 3 x the forward MACs of A + HE + HD + S (forward, bwd-data,
    bwd-weight); the all_reduce of the 2.6 MB gradient buffer is the only thing N > 1 adds."""
    import gc
    import torch
    from pcgcv1_amd import synthetic
    from pcgcv1_amd.models import spec
    from pcgcv1_amd.train_hyper import Trainer
    gc.unfreeze()
    tr = Trainer(synthetic.make_weights(seed=1300, profile="dense"), alpha=0.75, beta=3.0, lr=1e-5)
    x = torch.from_numpy(synthetic.make_cubes(seed=3, n_cubes=8)).cuda()
    for _ in range(3):
        tr.step(x)
    gc.collect()
    gc.freeze()
    out = {}
    for key, iou in (("ms_per_step", False), ("ms_per_step_with_iou", True)):      # the reference's loop classifies every step (216-226)
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.step(x, with_iou=iou)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        out[key] = round(1e3 * sorted(ts)[len(ts) // 2], 3)
    gflop = 3 * 2e-9 * 8 * sum(spec.macs_per_cube(net) for net in spec.NETS)
    tf = gflop / out["ms_per_step"]
    out.update({"workload": "train_hyper step, batch 8 x 64^3 (BASELINE configs[3] per GPU), alpha 0.75 beta 3, seeded weights",
                "cubes_per_s": round(8e3 / out["ms_per_step"], 1), "gflop_per_step": round(gflop, 1),
                "tflops": round(tf, 2), "frac_of_fp32_mfma_peak": round(tf / FP32_MFMA_PEAK_TFLOPS, 4)})
    del tr
    torch.cuda.empty_cache()
    return out


def _stream_block(transform, model, cubes, B, n=20):
    """A JOB of n clouds through transform.roundtrip_stream: the encode of cloud k + 1 runs (own thread, own HIP streams)
    while cloud k decodes, which fills the GPU's wait for the host at every encode -> decode hand-over.  Timed from a
    cold pipeline to the last reconstruction (fill and drain included).  NOT the headline: `value` stays one cloud at a
    time (encode, then decode, nothing else in flight), which is what the reference's command line does."""
    import torch
    for _o, _x in transform.roundtrip_stream((cubes for _ in range(3)), model, "bench"):
        pass
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _o, _x in transform.roundtrip_stream((cubes for _ in range(n)), model, "bench"):
        pass
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"clouds": n, "cubes_per_s": round(n * B / dt, 1), "ms_per_cloud": round(1e3 * dt / n, 3),
            "what": "transform.roundtrip_stream over %d copies of the cloud: compress_hyper of cloud k+1 overlaps decompress_hyper "
                    "of cloud k (two clouds in flight); same bytes, same reconstructions" % n}


def _large_block(transform, model, cubes, B, copies=8, n=3):
    """BASELINE configs[4]'s shape on one GPU: ONE cloud of thousands of cubes (here the headline cloud's cubes several times over)
    through the same compress_hyper + decompress_hyper: the encode -> decode hand-over is paid once per cloud, so the
    per-cube rate approaches what the kernels sustain."""
    import torch
    big = cubes.repeat(copies, 1, 1, 1, 1)
    nb = int(big.shape[0])

    def step():
        o = transform.compress_hyper(big, model, "bench")
        return transform.decompress_hyper(*o, model, "bench")
    step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del big
    torch.cuda.empty_cache()
    return {"cubes": nb, "cubes_per_s": round(nb * n / dt, 1), "ms_per_step": round(1e3 * dt / n, 3),
            "what": "one cloud of %d cubes (the headline cloud %d times over) per compress_hyper + decompress_hyper call" % (nb, copies)}


def _file_level(pts, B):
    """ply -> container files -> ply through the test.py CLI (ply parse, partition, voxelisation, codec, container, top-k,
    ply write), warm, in a scratch directory: the figure a user of the reference's command line sees."""
    import contextlib
    import io
    import shutil
    import tempfile
    from pcgcv1_amd import test as cli
    from pcgcv1_amd.dataprocess import inout_points as iop
    d = tempfile.mkdtemp(prefix="pcgc_bench_")
    cwd = os.getcwd()
    try:
        os.chdir(d)
        iop.write_ply_data("cloud_vox10.ply", pts)
        best = None
        for _ in range(5):
            with contextlib.redirect_stdout(io.StringIO()):
                t0 = time.perf_counter()
                cli.main(["compress", "cloud_vox10.ply", "--ckpt_dir=bench"])
                tc = time.perf_counter() - t0
                t0 = time.perf_counter()
                cli.main(["decompress", "compressed/cloud_vox10", "--ckpt_dir=bench"])
                td = time.perf_counter() - t0
            if os.environ.get("PCGC_BENCH_DEBUG"):
                sys.stderr.write("file_level: compress %.1f ms decompress %.1f ms\n" % (1e3 * tc, 1e3 * td))
            if best is None or tc + td < best[0] + best[1]:
                best = (tc, td)
        size = sum(os.path.getsize(os.path.join("compressed", f)) for f in os.listdir("compressed"))
        return {"cubes_per_s": round(B / (best[0] + best[1]), 1), "compress_s": round(best[0], 4), "decompress_s": round(best[1], 4),
                "file_bytes": size, "what": "python -m pcgcv1_amd.test compress + decompress, ply in -> 5 files -> ply out (best of 5, warm, in process)"}
    finally:
        os.chdir(cwd)
        shutil.rmtree(d, ignore_errors=True)


def _stage_times(transform, model, cubes):
    c = transform.get_codec(model, "bench")
    c.timers.clear()
    out = transform.compress_hyper(cubes, model, "bench", profile_stages=True)
    res = {"enc " + k: v for k, v in c.timers.items()}
    c.timers.clear()
    transform.decompress_hyper(*out, model, "bench", profile_stages=True)
    res.update({"dec " + k: v for k, v in c.timers.items()})
    c.timers.clear()
    return res


if __name__ == "__main__":
    main()
