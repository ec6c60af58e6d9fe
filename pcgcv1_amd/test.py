"""Command line of the reference's test.py (24-45 flags, 61-115 dispatch), same flags and defaults:

    python -m pcgcv1_amd.test compress  X.ply  --ckpt_dir=checkpoints/hyper/a6.00b3.00
    python -m pcgcv1_amd.test decompress compressed/X --ckpt_dir=checkpoints/hyper/a6.00b3.00

compress writes ./compressed/<basename>.{strings,strings_head,strings_hyper,pointnums,cubepos};
decompress writes <name>_rec.ply.  compress --colors=raht --color_qstep=Q (a coloured ply) adds <basename>.colors, the colours
of the decoded points (pcgcv1_amd/colorcodec.py); decompress finds that file and writes a coloured ply;
--color_target=psnr:38 or bpp:0.6 instead of --color_qstep lets the encoder choose the step for a luma PSNR or a size.  --ckpt_dir additionally accepts "synthetic[:seed[:profile]]"
(checkpoint.py).  --gpu=0 is rejected: this build has no CPU path; --gpu=N shards the cubes over N GPUs
(one rank per GPU over RCCL, pcgcv1_amd/sharding.py; same files as one GPU).  compress --voxelize=BITS (or --voxel_size=S) takes a
raw scan (float coordinates, several points per voxel; pcgcv1_amd/ingest.py) and adds <basename>.frame; decompress finds that
file and writes the points in the scan's own coordinates.
"""
import argparse
import importlib
import os
import time


# flag, type, default, meaning — names and defaults are the reference's (test.py:24-45)
_FLAGS = [
    ("mode", str, "hyper", "entropy model: 'hyper' (hyperprior) or 'factorized'"),
    ("modelname", str, "models.model_voxception", "module with the transforms: models.model_voxception | models.model_simple"),
    ("ckpt_dir", str, "", "TensorFlow checkpoint directory, weights.npz directory, or synthetic[:seed[:profile]]"),
    ("scale", float, 1.0, "coordinates are multiplied by this before partitioning (and divided back on output)"),
    ("cube_size", int, 64, "edge of the cubes the cloud is cut into"),
    ("min_num", int, 64, "cubes with fewer points are dropped"),
    ("rho", float, 1.0, "output points per cube = rho x the stored point count"),
    ("pointnums", str, "count", "what .pointnums holds: 'count' = each cube's point count (the reference's); 'd1' = the counts "
                                "that give the decoder at rho = 1 the smallest cube-local D1 (pcgcv1_amd/pointnums.py); 'd2' = "
                                "the same for the point-to-plane error D2, with the normals of the ply (nx ny nz) or of "
                                "--estimate_normals"),
    ("gpu", int, 1, "GPUs to use: 1 = this process; N > 1 = the cube list sharded over N ranks, one per GPU (started here "
                    "unless a launcher already set WORLD_SIZE); 0 is refused: there is no CPU path"),
    ("colors_from", str, "", "decompress only: the ORIGINAL coloured ply; the written _rec.ply then carries its colours transferred "
                             "onto the decoded points (pcgcv1_amd/recolor.py).  An encoder-side / evaluation tool: a real decoder "
                             "does not have this file.  Colours that travel in the bitstream: compress --colors=raht"),
    ("colors", str, "none", "compress only: 'raht' = code the colours of the decoded points (the input's, transferred onto the "
                            "encoder's own reconstruction at rho = 1) into <name>.colors with the RAHT codec "
                            "(pcgcv1_amd/colorcodec.py); decompress then writes a coloured ply.  'none' = geometry only"),
    ("color_qstep", float, 4.0, "quantiser step of --colors=raht (all three YCoCg channels); larger = fewer bits"),
    ("color_coder", str, "range", "entropy coder of --colors=raht: 'range' = stream version 1 (the host's range coder); 'rans' = version "
                                  "2, chunked interleaved rANS coded and decoded on the GPU.  decompress reads either"),
    ("color_target", str, "", "rate control of --colors=raht instead of --color_qstep: 'psnr:38' = the largest step of the grid "
                              "2^(j/8) whose decoded luma (BT.709 Y) PSNR is at least 38 dB; 'bpp:0.6' = the smallest step whose "
                              "<name>.colors holds at most 0.6 bits per input point.  Empty: --color_qstep as given"),
]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("command", choices=("compress", "decompress"), help="compress: .ply -> ./compressed/<name>.*; "
                                                                         "decompress: those files -> <name>_rec.ply")
    ap.add_argument("input", nargs="?", help="point cloud (.ply) or compressed file stem")
    ap.add_argument("output", nargs="?", help="output stem / .ply (derived from the input when omitted)")
    for name, typ, default, meaning in _FLAGS:
        ap.add_argument("--" + name, type=typ, default=default, help=meaning,
                        **({"choices": ("count", "d1", "d2")} if name == "pointnums" else {"choices": ("none", "raht")} if name == "colors" else
                           {"choices": ("range", "rans")} if name == "color_coder" else {}))
    ap.add_argument("--estimate_normals", action="store_true",
                    help="compress --pointnums=d2 with a ply that has no normals: estimate them (radius 10, 20 neighbours, as eval does)")
    ap.add_argument("--voxelize", type=int, default=0, metavar="BITS",
                    help="compress only: the input is a raw scan (float coordinates, any number of points per voxel); put it on a grid "
                         "of 2^BITS cells per axis first (pcgcv1_amd/ingest.py), merged colours and normals feeding --colors=raht and "
                         "--pointnums=d2, and write <name>.frame so that decompress returns the scan's own coordinates")
    ap.add_argument("--voxel_size", type=float, default=0.0, metavar="S",
                    help="compress only: as --voxelize, with voxels of edge S in the scan's units instead of a bit count")
    from .clean import add_clean_argument, check_clean_argument
    add_clean_argument(ap)
    from .smooth import add_smooth_argument, check_smooth_argument
    add_smooth_argument(ap)
    ap.add_argument("--render", default="", metavar="X.png",
                    help="decompress only: also draw the cloud just written into this png (pcgcv1_amd/render.py, default view and size)")
    ap.add_argument("--mesh", default="", metavar="X.obj",
                    help="decompress only: also reconstruct a triangle mesh (.obj or .off) from the cloud just written "
                         "(pcgcv1_amd/surface.py: estimated normals, default radius and orientation)")
    ap.add_argument("--mesh_simplify", type=int, default=None, metavar="CELL",
                    help="with --mesh: simplify the mesh on the GPU before it is written, one vertex per cube of CELL voxels (1..64) "
                         "placed by its quadric (pcgcv1_amd/surface.py: simplify)")
    args = ap.parse_args(argv)
    check_clean_argument(ap, args)
    check_smooth_argument(ap, args)
    if args.mesh_simplify is not None:
        from .surface import check_cell
        try:
            check_cell(args.mesh_simplify)
        except ValueError as e:
            ap.error(str(e))
        if not args.mesh:
            ap.error("--mesh_simplify=%d simplifies the mesh --mesh writes: give --mesh X.obj too" % args.mesh_simplify)
    if args.smooth and (args.command != "compress" or not (args.voxelize or args.voxel_size)):
        ap.error("--smooth moves the float points of a raw scan: it belongs to compress --voxelize or --voxel_size (a voxelised "
                 "ply has no float points)")
    if args.clean and args.command != "compress":
        ap.error("--clean belongs to compress: decompress writes what the stream holds")
    if args.clean and args.scale != 1:
        ap.error("--clean filters the voxels of the grid as it is: --scale must be 1 (got %g)" % args.scale)
    if args.clean and (args.gpu > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1):
        ap.error("multi-GPU runs read a cleaned ply (--clean runs on one GPU)")
    if args.color_target:                                 # with the other argument errors, before anything is loaded
        from .colorcodec import parse_target
        try:
            parse_target(args.color_target)
        except ValueError as e:
            ap.error(str(e))
        if args.colors != "raht":
            ap.error("--color_target=%s steers the quantiser of --colors=raht: give both" % args.color_target)
        if args.color_qstep != ap.get_default("color_qstep"):
            ap.error("--color_target=%s chooses the step itself: leave --color_qstep=%g out" % (args.color_target, args.color_qstep))
    if args.command == "compress" and args.pointnums == "d2" and not args.estimate_normals and not _ply_has_normals(args.input):
        # with the other argument errors, before anything is loaded: d2 has nothing to measure against without normals
        ap.error("--pointnums=d2 needs normals: %s has no nx ny nz properties (or cannot be read); write them into the ply, or "
                 "pass --estimate_normals to estimate them (radius 10, 20 neighbours)" % args.input)
    # the line every run prints: the ingest flags show up in it only when they are given
    print(argparse.Namespace(**{k: v for k, v in vars(args).items() if k not in ("voxelize", "voxel_size", "clean", "smooth", "mesh_simplify") or v}))
    return args


def _ply_has_normals(filename):
    """whether the ply's header declares nx, ny and nz (False for a file that is missing or has no header)"""
    try:
        with open(filename, "rb") as f:
            head = f.read(1 << 16)
    except (OSError, TypeError):
        return False
    end = head.find(b"end_header")
    if end < 0:
        return False
    props = {ln.split()[-1] for ln in head[:end].split(b"\n") if ln.strip().startswith(b"property")}
    return {b"nx", b"ny", b"nz"} <= props


def _import_model(name):
    if name.startswith("models."):
        name = "pcgcv1_amd." + name
    return importlib.import_module(name)


def _report(model, ckpt_dir, t0, also=""):
    import torch
    from .transform import get_codec
    torch.cuda.synchronize()
    p = get_codec(model, ckpt_dir).last_path
    print("{}{}: {}s ({} cubes, {} host pipeline{})".format(p.get("call"), also, round(time.time() - t0, 4), p.get("cubes"),
                                                           p.get("pipelines"), "" if p.get("pipelines") == 1 else "s"))


def _d1_counts(cubes, logits, points_numbers):
    """--pointnums=d1: the counts pointnums.optimize_points_numbers picks for these logits, with a line on what it chose"""
    from .pointnums import optimize_points_numbers
    counts, rep = optimize_points_numbers(cubes, logits, points_numbers)
    print("pointnums d1: chose {} {}; cube-local D1 mse {:.6g} -> {:.6g} (PSNR {:.4f} -> {:.4f} dB at peak 1023)".format(
        rep["choice"][0], rep["choice"][1], rep["F_count"], rep["F_chosen"], rep["psnr_count"], rep["psnr_chosen"]))
    return counts


def _load_normals(args):
    """--pointnums=d2: (points, normals) of the input, before any other work: the ply's own nx ny nz, or estimated ones"""
    from .dataprocess.inout_points import load_ply_normals
    points, normals = load_ply_normals(args.input)
    if normals is None:
        if not args.estimate_normals:
            raise SystemExit("--pointnums=d2 needs normals: %s has no nx ny nz properties; write them into the ply, or pass "
                             "--estimate_normals to estimate them (radius 10, 20 neighbours)" % args.input)
        from .metrics import estimate_normals
        normals = estimate_normals(points, 10, 20)
    return points, normals


def _d2_counts(args, cubes, logits, points_numbers, cube_positions, source):
    """--pointnums=d2: the normals go to the cubes' occupied voxels, then the optimiser runs on the point-to-plane curves"""
    from .pointnums import optimize_points_numbers, voxel_normals
    vn = voxel_normals(source[0], source[1], cube_positions, args.scale, args.cube_size)
    counts, rep = optimize_points_numbers(cubes, logits, points_numbers, metric="d2", normals=vn)
    print("pointnums d2: chose {} {}; cube-local D2 mse {:.6g} -> {:.6g} (PSNR {:.4f} -> {:.4f} dB at peak 1023)".format(
        rep["choice"][0], rep["choice"][1], rep["F_count"], rep["F_chosen"], rep["psnr_count"], rep["psnr_chosen"]))
    return counts


def _main_sharded(args, world):
    """One process per GPU (`python -m torch.distributed.run --nproc-per-node N -m pcgcv1_amd.test ...`): the cube
    list is split over the ranks (pcgcv1_amd/sharding.py), rank 0 reads and writes the files.  Same files as one GPU."""
    import torch
    import torch.distributed as dist
    from . import sharding
    from .dataprocess import inout_bitstream as bs
    from .process import postprocess_masks, preprocess
    if args.mode != "hyper":
        raise SystemExit("multi-GPU runs are implemented for --mode=hyper")
    if args.pointnums != "count":
        raise SystemExit("multi-GPU runs write --pointnums=count only (--pointnums=d1 and d2 run on one GPU)")
    rank = int(os.environ.get("RANK", "0"))
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count()))
    if not dist.is_initialized():
        dist.init_process_group(os.environ.get("PCGC_BACKEND", "nccl"))
    ops = sharding.HipOps(_import_model(args.modelname), args.ckpt_dir)
    if args.command == "compress":
        if not args.output:
            args.output = os.path.split(args.input)[-1][:-4]
        # every rank parses + partitions the cloud (host, cheap) but voxelises and uploads only its own block of cubes
        cubes, cube_positions, nums_local = preprocess(args.input, args.scale, args.cube_size, args.min_num, verbose=rank == 0,
                                                       block=(rank, world))
        stream = sharding.compress_hyper_sharded(cubes, ops, total=len(cube_positions), points_numbers=nums_local)
        if rank == 0:
            y_strings, y_min_vs, y_max_vs, y_shape, z_strings, z_min_v, z_max_v, z_shape, points_numbers = stream
            bs.write_binary_files_hyper(args.output, y_strings, z_strings, points_numbers, cube_positions, y_min_vs, y_max_vs,
                                        y_shape, z_min_v, z_max_v, z_shape, rootdir='./compressed')
    else:
        rootdir, filename = os.path.split(args.input)
        if not args.output:
            args.output = filename + "_rec.ply"
        stream = nums = pos = None
        if rank == 0:
            (y_strings, z_strings, nums, pos, y_min_vs, y_max_vs, y_shape, z_min_v, z_max_v,
             z_shape) = bs.read_binary_files_hyper(filename, rootdir)
            stream = (y_strings, y_min_vs, y_max_vs, y_shape, z_strings, z_min_v, z_max_v, z_shape)
        masks = sharding.decompress_hyper_sharded(stream, ops, points_numbers=nums, rho=args.rho)
        if rank == 0:
            postprocess_masks(args.output, masks, pos, args.scale, args.cube_size)
    dist.barrier()


def _self_launch(argv, n):
    """--gpu=N without a launcher: the N ranks as a child `torch.distributed.run` of this module, started before this
    process has touched the GPU; exits with the child's code (non-zero if any rank failed)."""
    import subprocess
    import sys
    # --standalone: torchrun hosts the c10d rendezvous itself on a port IT binds and keeps (a port probed here by bind / close
    # could be taken by another process before the ranks meet)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1", "--nproc-per-node", str(n),
           "-m", "pcgcv1_amd.test"] + list(sys.argv[1:] if argv is None else argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    return subprocess.run(cmd, env=env).returncode


def main(argv=None):
    args = parse_args(argv)
    if not args.render and not args.mesh:
        return _main(args, argv)
    several = args.gpu > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1
    if args.render and args.command != "decompress":
        raise SystemExit("--render belongs to decompress: it draws the cloud decompress has just written")
    if args.render and several:
        raise SystemExit("--render runs on one GPU")
    if args.mesh:
        if args.command != "decompress":
            raise SystemExit("--mesh belongs to decompress: it reconstructs a surface from the cloud decompress has just written")
        if several:
            raise SystemExit("--mesh runs on one GPU")
        from .surface import check_output
        try:
            check_output(args.mesh)
        except ValueError as e:
            raise SystemExit(str(e))
    _main(args, argv)
    if args.render:
        _render_output(args)
    if args.mesh:
        _mesh_output(args)


def _render_output(args):
    """--render: the ply decompress has just written (args.output), default view and size, in its own colours if it has any"""
    from .dataprocess.inout_points import load_ply_colors
    from .render import render, write_png
    t0 = time.time()
    points, colors = load_ply_colors(args.output, as_float=True)
    write_png(args.render, render(points, colors))
    print("Render {} to {}: {}s ({} points)".format(args.output, args.render, round(time.time() - t0, 4), len(points)))


def _mesh_output(args):
    """--mesh: a surface from the ply decompress has just written (args.output): estimated normals, default radius and orientation.
    Where <name>.frame put the cloud into a scan's units, the voxels are taken back to the grid and the mesh is written in those units.
    --mesh_simplify CELL: the mesh is simplified on the device first (surface.simplify), and a second line reports it."""
    import numpy as np
    from .dataprocess.inout_points import load_ply_scan
    from .surface import mesh_file
    t0 = time.time()
    points, _, _ = load_ply_scan(args.output)
    frame = None
    if os.path.exists(args.input + ".frame"):
        from .ingest import read_frame
        frame = read_frame(args.input + ".frame")
        points = (points - frame.origin) / frame.step
    voxels = np.unique(np.rint(points).astype(np.int32), axis=0)
    print(mesh_file(voxels, None, args.mesh, frame=frame, simplify=args.mesh_simplify))
    print("Mesh {} to {}: {}s".format(args.output, args.mesh, round(time.time() - t0, 4)))


def _main(args, argv):
    if args.gpu < 1:
        raise SystemExit("--gpu=0: this build runs the hot path on an MI355X only (no CPU fallback)")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.voxelize or args.voxel_size:
        if args.voxelize and args.voxel_size:
            raise SystemExit("--voxelize=%d and --voxel_size=%g both choose the grid of the scan: give one of them" % (args.voxelize, args.voxel_size))
        if args.command != "compress":
            raise SystemExit("--voxelize and --voxel_size belong to compress: decompress reads the frame from <name>.frame")
        if args.scale != 1:
            raise SystemExit("--voxelize and --voxel_size put the scan on the grid themselves: --scale must be 1 (got %g)" % args.scale)
        if args.gpu > 1 or world > 1:
            raise SystemExit("multi-GPU runs read a voxelised ply (--voxelize and --voxel_size run on one GPU)")
        if not (1 <= args.voxelize <= 12 if args.voxelize else args.voxel_size > 0):
            raise SystemExit("--voxelize takes 1..12 bits, --voxel_size a positive edge (got %s)" % (args.voxelize or args.voxel_size))
    if args.command == "decompress" and args.input and os.path.exists(args.input + ".frame"):
        why = "%s.frame maps the grid of the scale = 1 reconstruction back to the scan, on one GPU" % args.input
        if args.scale != 1:
            raise SystemExit("--scale=%g: %s" % (args.scale, why))
        if args.gpu > 1 or world > 1:
            raise SystemExit("--gpu=%d: %s" % (max(args.gpu, world), why))
    if (args.gpu > 1 or world > 1) and args.pointnums != "count":
        raise SystemExit("multi-GPU runs write --pointnums=count only (--pointnums=d1 and d2 run on one GPU)")
    if args.estimate_normals and (args.command != "compress" or args.pointnums != "d2"):
        raise SystemExit("--estimate_normals belongs to compress --pointnums=d2")
    if (args.gpu > 1 or world > 1) and args.colors_from:
        raise SystemExit("multi-GPU runs write geometry only (--colors_from runs on one GPU)")
    if args.colors_from and args.command != "decompress":
        raise SystemExit("--colors_from belongs to decompress: compress reads geometry only, the bitstream holds no colours")
    if args.color_coder != "range" and args.colors != "raht":
        raise SystemExit("--color_coder=%s chooses the entropy coder of --colors=raht: give both (decompress reads the coder from the file)"
                         % args.color_coder)
    if args.colors != "none":
        if args.command != "compress":
            raise SystemExit("--colors belongs to compress: decompress decodes <name>.colors whenever the file is there")
        if args.gpu > 1 or world > 1:
            raise SystemExit("multi-GPU runs write geometry only (--colors=raht runs on one GPU)")
        if args.scale != 1:
            raise SystemExit("--colors=raht codes the colours of a voxelised reconstruction: --scale must be 1 (got %g)" % args.scale)
        if not (args.color_qstep > 0):
            raise SystemExit("--color_qstep must be positive (got %g)" % args.color_qstep)
    if args.command == "decompress" and args.input and os.path.exists(args.input + ".colors"):
        why = "%s.colors holds the colours of the rho = 1, scale = 1 reconstruction, decoded on one GPU" % args.input
        if args.rho != 1:
            raise SystemExit("--rho=%g: %s (decode with --rho=1, or remove the file for geometry only)" % (args.rho, why))
        if args.scale != 1:
            raise SystemExit("--scale=%g: %s" % (args.scale, why))
        if args.colors_from:
            raise SystemExit("--colors_from: %s; the stream's own colours are written, no original is needed" % why)
        if args.gpu > 1 or world > 1:
            raise SystemExit("--gpu=%d: %s" % (max(args.gpu, world), why))
    if args.gpu > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(_self_launch(argv, args.gpu))
    if args.gpu > 1 and world != args.gpu:                 # e.g. --gpu=8 under `torchrun --nproc-per-node 1`: never silently one GPU
        raise SystemExit("WORLD_SIZE=%d but --gpu=%d" % (world, args.gpu))
    if world > 1:
        return _main_sharded(args, world)
    from .process import preprocess, postprocess, StreamedPostprocess
    from .transform import compress_hyper, decompress_hyper, compress_factorized, decompress_factorized
    from .dataprocess import inout_bitstream as bs
    model = _import_model(args.modelname)
    stage_times = os.environ.get("PCGC_STAGE_TIMES", "0") == "1"
    if args.command == "compress":
        if not args.output:
            args.output = os.path.split(args.input)[-1][:-4]
        coded_colors = args.colors == "raht"
        optimised = args.pointnums != "count"
        points = frame = None
        if args.voxelize or args.voxel_size:      # a raw scan: its merged points, colours and normals stand in for the file's
            points, src_points, src_colors, source, frame = _voxelize_input(args, coded_colors)
        else:
            if coded_colors:                      # before any GPU work: a ply without colours is refused by name
                from .recolor import load_source
                src_points, src_colors = load_source(args.input)
            if args.pointnums == "d2":            # likewise: a ply without normals is refused before any GPU work
                source = _load_normals(args)
            if args.clean:                        # a voxelised ply: its outlier voxels go, with their colours and normals
                points, src_points, src_colors, source = _clean_input(args, src_points if coded_colors else None,
                                                                      src_colors if coded_colors else None,
                                                                      source if args.pointnums == "d2" else None)
        cubes, cube_positions, points_numbers = preprocess(args.input, args.scale, args.cube_size, args.min_num, points=points)
        logits = None
        if args.mode == "factorized":
            strings, min_v, max_v, shape = compress_factorized(cubes, model, args.ckpt_dir, verbose=True)
            if optimised or coded_colors:                        # the decoder's logits: decode the strings as decompress does
                logits = decompress_factorized(strings, min_v, max_v, shape, model, args.ckpt_dir)
            if args.pointnums == "d1":
                points_numbers = _d1_counts(cubes, logits, points_numbers)
            elif args.pointnums == "d2":
                points_numbers = _d2_counts(args, cubes, logits, points_numbers, cube_positions, source)
            bs.write_binary_files_factorized(args.output, strings, points_numbers, cube_positions, min_v, max_v, shape,
                                             rootdir='./compressed', frame=frame)
        else:
            # the batched, two-pipeline path bench.py times; PCGC_STAGE_TIMES=1 prints the reference's per-stage times
            # instead (transform.py:121-171), which serialises the stages
            t0 = time.time()
            from . import _lib
            # host work under the GPU's: the cube positions are coded (0.6 ms of Python, interpreter lock held) once the encoder's
            # pipeline threads have queued their kernels and sit in event waits — started at once it delayed THEIR start by as much
            # (tools/exp/t_cli_timeline.py)
            def _cubepos():
                time.sleep(0.003)
                return bs.encode_cube_positions(cube_positions)
            cubepos = _lib.workers("job").submit(_cubepos)
            if optimised or coded_colors:                        # the encoder-side reconstruction is what the decoder will compute
                out = compress_hyper(cubes, model, args.ckpt_dir, decompress=True, verbose=stage_times)
                logits = out[8]
                if args.pointnums == "d1":
                    points_numbers = _d1_counts(cubes, logits, points_numbers)
                elif args.pointnums == "d2":
                    points_numbers = _d2_counts(args, cubes, logits, points_numbers, cube_positions, source)
                out = out[:8]
            else:
                out = compress_hyper(cubes, model, args.ckpt_dir, verbose=stage_times)
            (y_strings, y_min_vs, y_max_vs, y_shape, z_strings, z_min_v, z_max_v, z_shape) = out
            _report(model, args.ckpt_dir, t0)
            bs.write_binary_files_hyper(args.output, y_strings, z_strings, points_numbers, cube_positions, y_min_vs,
                                        y_max_vs, y_shape, z_min_v, z_max_v, z_shape, rootdir='./compressed',
                                        cubepos=cubepos.result(), frame=frame)
        if coded_colors:
            _write_colors(args, logits, points_numbers, cube_positions, src_points, src_colors)
    else:
        rootdir, filename = os.path.split(args.input)
        if not args.output:
            args.output = filename + "_rec.ply"
        colors_file = args.input + ".colors" if os.path.exists(args.input + ".colors") else ""
        frame = None
        if os.path.exists(args.input + ".frame"):        # the cloud was voxelised from a scan: its own coordinates go out
            from .ingest import read_frame
            frame = read_frame(args.input + ".frame")
        if args.mode == "factorized":
            strings, points_numbers, cube_positions, min_v, max_v, shape = bs.read_binary_files_factorized(filename, rootdir)
            cubes = decompress_factorized(strings, min_v, max_v, shape, model, args.ckpt_dir, verbose=True)
        else:
            (y_strings, z_strings, points_numbers, cube_positions, y_min_vs, y_max_vs, y_shape, z_min_v, z_max_v,
             z_shape) = bs.read_binary_files_hyper(filename, rootdir)
            t0 = time.time()
            # the tail (top-k, points, text, file) follows the decoder slice by slice instead of waiting for the last cube;
            # PCGC_STREAM_TAIL=0 / --scale != 1 / PCGC_STAGE_TIMES=1: postprocess on the whole batch, as the reference does
            tail = None
            if args.scale == 1 and not stage_times and os.environ.get("PCGC_STREAM_TAIL", "1") != "0" and not args.colors_from and not colors_file and frame is None:
                tail = StreamedPostprocess(args.output, points_numbers, cube_positions, args.scale, args.cube_size, args.rho)
            cubes = decompress_hyper(y_strings, y_min_vs, y_max_vs, y_shape, z_strings, z_min_v, z_max_v, z_shape, model,
                                     args.ckpt_dir, verbose=stage_times, on_slice=tail)
            if tail is not None:
                print('===== Post process =====')
                tail.finish()
                _report(model, args.ckpt_dir, t0, " + post process")
                return
            _report(model, args.ckpt_dir, t0)
        if args.colors_from:
            return _write_recolored(args, cubes, points_numbers, cube_positions, frame)
        if colors_file:
            return _write_decoded_colors(args, cubes, points_numbers, cube_positions, colors_file, frame)
        if frame is not None:
            return _write_in_frame(args, cubes, points_numbers, cube_positions, frame)
        postprocess(args.output, cubes, points_numbers, cube_positions, args.scale, args.cube_size, args.rho)


def _voxelize_input(args, coded_colors):
    """--voxelize / --voxel_size: the scan read as it is and put on its grid in memory (pcgcv1_amd/ingest.py) -> (points, colour
    source points, colour source colours, (points, normals) for d2 or None, the 40 bytes of <name>.frame).  What the scan
    lacks is refused by name before any GPU work."""
    import numpy as np
    from . import ingest
    from .dataprocess.inout_points import load_ply_scan
    t0 = time.time()
    scan, colors, normals = load_ply_scan(args.input)
    if coded_colors and colors is None:
        raise SystemExit("%s has no colour properties (red green blue): nothing to transfer" % args.input)
    if args.pointnums == "d2" and normals is None and not args.estimate_normals:
        raise SystemExit("--pointnums=d2 needs normals: %s has no nx ny nz properties; write them into the ply, or pass "
                         "--estimate_normals to estimate them (radius 10, 20 neighbours)" % args.input)
    try:
        (points, colors, normals, counts, frame, n_dropped), cleaned = ingest.voxelize_scan_report(
            scan, colors if coded_colors else None, normals if args.pointnums == "d2" else None,
            bits=args.voxelize or None, voxel_size=args.voxel_size or None, clean=args.clean, smooth=args.smooth)
    except ValueError as e:
        raise SystemExit("%s: %s" % (args.input, e))
    print(ingest.summary_line(len(scan), n_dropped, counts, frame))
    if cleaned:
        print(cleaned)
    print("Read and voxelise {}: {}s".format(args.input, round(time.time() - t0, 4)))
    source = None
    if args.pointnums == "d2":
        if normals is None:
            from .metrics import estimate_normals
            normals = estimate_normals(points, 10, 20)
        else:                                     # as the voxelised ply would hand them on: six decimals (write_ply_normals)
            normals = np.round(normals.astype("float"), 6).astype(np.float32)
        source = (points, normals)
    return points, points, colors, source, ingest.frame_bytes(frame)


def _clean_input(args, src_points, src_colors, source):
    """--clean on a voxelised ply (pcgcv1_amd/clean.py) -> (points, colour source points, colours, (points, normals) for d2):
    the file's rows that the filters keep.  The colour and normal rows are the file's rows, so one mask serves them all."""
    import numpy as np
    from . import clean
    from .dataprocess.inout_points import load_ply_data
    t0 = time.time()
    points = load_ply_data(args.input)
    try:
        if len(np.unique(points, axis=0)) != len(points):
            raise ValueError("a voxel holds several points: --clean reads one point per voxel (--voxelize merges a raw scan)")
        report = []
        kept, _, _, _, mask = clean.clean_cloud(points, None, None, None, clean.bits_for(points), args.clean, report)
    except ValueError as e:
        raise SystemExit("%s: %s" % (args.input, e))
    print(clean.summary_line(args.clean, len(points), len(points) - len(kept), clean.n_cubes(points), clean.n_cubes(kept)))
    for line in report:                           # a component filter's own line (clean.components_line)
        print(line)
    print("Read and clean {}: {}s".format(args.input, round(time.time() - t0, 4)))
    if src_points is not None:
        src_points, src_colors = src_points[mask], src_colors[mask]
    if source is not None:
        source = (source[0][mask], source[1][mask])
    return kept, src_points, src_colors, source


def _write_in_frame(args, cubes, points_numbers, cube_positions, frame):
    """<name>.frame is there: the decoded points (postprocess's, in its order) in the scan's own coordinates"""
    from .dataprocess.inout_points import write_ply_data
    from .ingest import apply_frame
    from .process import postprocess_points
    print('===== Post process =====')
    t0 = time.time()
    pts = postprocess_points(cubes, points_numbers, cube_positions, args.scale, args.cube_size, args.rho)
    write_ply_data(args.output, apply_frame(pts, frame))
    print("Apply {}.frame and write {}: {}s ({} points, step {!r})".format(args.input, args.output, round(time.time() - t0, 4), len(pts),
                                                                           frame.step))


def _write_recolored(args, cubes, points_numbers, cube_positions, frame=None):
    """--colors_from: the decoded points (the ones postprocess would write, in its order) with the original's colours"""
    from .dataprocess.inout_points import write_ply_colors
    from .process import postprocess_points
    from .recolor import load_source, recolor
    print('===== Post process =====')
    t0 = time.time()
    src_points, src_colors = load_source(args.colors_from)
    pts = postprocess_points(cubes, points_numbers, cube_positions, args.scale, args.cube_size, args.rho)
    colors, counts = recolor(src_points, src_colors, pts, return_counts=True)
    write_ply_colors(args.output, pts if frame is None else _in_frame(pts, frame), colors)
    print("Recolour from {} and write {}: {}s ({} of {} points coloured from their own nearest source points)".format(
        args.colors_from, args.output, round(time.time() - t0, 4), int((counts == 0).sum()), len(pts)))


def _write_colors(args, logits, points_numbers, cube_positions, src_points, src_colors):
    """--colors=raht: the points the decoder will write at rho = 1 (from the encoder's own decode), the input's colours transferred
    onto them, coded into compressed/<name>.colors"""
    import numpy as np
    from .colorcodec import encode_colors, write_colors_file
    from .process import postprocess_points
    from .recolor import recolor
    t0 = time.time()
    pts = np.asarray(postprocess_points(logits, points_numbers, cube_positions, 1, args.cube_size, 1)).astype(np.int32)
    name = os.path.join("./compressed", args.output + ".colors")
    if args.color_target:
        from .colorcodec import encode_colors_target, parse_target
        kind, value = parse_target(args.color_target)
        if kind == "bpp":                         # per INPUT point here, as the geometry's bpp; the codec counts the points it codes
            value = value * len(src_points) / len(pts)
        data, rep = encode_colors_target(pts, recolor(src_points, src_colors, pts), coder=args.color_coder, **{kind: value})
        write_colors_file(name, data)
        print("colors raht, target {}: color_qstep {:g} (grid notch {}), luma PSNR {:.4f} dB, {} bytes ({:.4f} bits per input point{}), "
              "{} probes, {} real encodes, for {} decoded points -> {}: {}s".format(
                  args.color_target, rep["qstep"], rep["j"], rep["psnr_y"], len(data), 8.0 * len(data) / len(src_points),
                  ", rANS" if args.color_coder == "rans" else "", rep["probes"], rep["real_encodes"], len(pts), name, round(time.time() - t0, 4)))
        return
    data = encode_colors(pts, recolor(src_points, src_colors, pts), args.color_qstep, coder=args.color_coder)
    write_colors_file(name, data)
    print("colors raht: {} bytes ({:.4f} bits per input point, color_qstep {:g}{}) for {} decoded points -> {}: {}s".format(
        len(data), 8.0 * len(data) / len(src_points), args.color_qstep, ", rANS" if args.color_coder == "rans" else "", len(pts), name,
        round(time.time() - t0, 4)))


def _in_frame(pts, frame):
    from .ingest import apply_frame
    return apply_frame(pts, frame)


def _write_decoded_colors(args, cubes, points_numbers, cube_positions, colors_file, frame=None):
    """<name>.colors is there: the decoded points (postprocess's, in its order) with the colours the stream holds"""
    import numpy as np
    from .colorcodec import decode_colors, read_colors_file
    from .dataprocess.inout_points import write_ply_colors
    from .process import postprocess_points
    print('===== Post process =====')
    t0 = time.time()
    pts = postprocess_points(cubes, points_numbers, cube_positions, args.scale, args.cube_size, args.rho)
    colors = decode_colors(np.asarray(pts).astype(np.int32), read_colors_file(colors_file))
    write_ply_colors(args.output, pts if frame is None else _in_frame(pts, frame), colors)
    print("Decode {} and write {}: {}s ({} points)".format(colors_file, args.output, round(time.time() - t0, 4), len(pts)))


if __name__ == "__main__":
    main()
