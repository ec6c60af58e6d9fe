"""What surface reconstruction costs: the parts of pcgcv1_amd.surface.reconstruct one by one and the whole call, with normals from
metrics.estimate_normals, on two clouds:
  * sparse: tools/register_bench.py's scan (1 000 000 points of ingest_bench's sphere, squeezed and with a bump) at 10 bits, about
    800 k voxels, the size of the codec's bench cloud.  A million points over a surface of more than a million voxels leave a
    cloud full of holes: many components, few rounds, a mesh in pieces;
  * dense: 4 000 000 points of the same surface at 9 bits, a closed sheet that the propagation has to walk across;
then the parts of surface.simplify at cell 2 on the mesh just built and reconstruct(simplify=2) next to reconstruct(),
then the parts of metrics.mesh_error, the voxels against the mesh just built and against the mesh simplified at cell 2, next to
one direction of pc_error_float's search on the same cloud and reconstruct(simplify=2, error=True),
and for scale the numpy rule (tests/_surface_ref.py) next to the device on a cloud the rule finishes in seconds (a sphere of
radius 50 at 7 bits).

    python tools/surface_bench.py [--repeats 7] > profiles/surface_bench.txt
    python tools/surface_bench.py --mesh_error_only >> profiles/surface_bench.txt     # the mesh_error lines alone

Per line: two warm-up calls, then the median (and the range) of `repeats` calls, each timed with a host clock around the call
and a device synchronise."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from components_bench import voxels                                      # noqa: E402
from ingest_bench import line, timed                                      # noqa: E402
from register_bench import make_scan                                      # noqa: E402
from pcgcv1_amd import _lib, metrics, surface                            # noqa: E402


def mesh_error_lines(p, nr, bits, radius, meshes, repeats):
    """the parts of metrics.mesh_error for the voxels p against each (label, vertices, triangles), as _mesh_error_device chains
    them, then the whole call; its yardsticks on the same cloud"""
    inf = float("inf")
    for label, v, t in meshes:
        (pd, vd, td, lo, hi), ts = timed(lambda: metrics._mesh_error_input(p, v, t), repeats)
        line("mesh_error, %s: input checks, bounds" % label, ts, "   %d points, %d triangles" % (len(pd), len(td)))
        s = metrics._MeshSearch(vd, td, lo, hi)
        _, ts = timed(lambda: (s.choose(), s.emit()), repeats)
        line("mesh_error, %s: count, scan, emit, sort" % label, ts, "   cell edge %d, %d cells per axis, %d pairs (%.2f per triangle)" % (
            s.cells[0], s.cells[4], s.pairs, s.pairs / len(td)))
        _, ts = timed(lambda: s.prepare(len(pd)), repeats)
        line("mesh_error, %s: prepare (pack, cells)" % label, ts)
        order, ts = timed(lambda: s.order(pd), repeats)
        line("mesh_error, %s: the points by cell" % label, ts)
        (out, _, _), ts = timed(lambda: s.query(pd, order, inf), repeats)
        mse, top, far, evaluated = out.tolist()
        line("mesh_error, %s: query, one thread per point" % label, ts, "   %.1f candidates per point; rms %.4f, max %.4f voxels" % (
            evaluated / len(pd), np.sqrt(mse), np.sqrt(top)))
        _, ts = timed(lambda: s.query(pd, None, inf), repeats)
        line("mesh_error, %s: query, the points as they come" % label, ts)
        fig, ts = timed(lambda: metrics.mesh_error(p, v, t), repeats)
        line("mesh_error, %s: the whole call" % label, ts)
        del s, pd, vd, td, order
    # one direction of pc_error_float's search, the voxels against the vertices of the last mesh and against themselves
    cloud = p.to(torch.float32).contiguous()
    lib = _lib.hip()
    for label, q in (("the vertices of that mesh", meshes[-1][1].to(torch.float32).cpu().numpy()), ("the cloud itself", cloud.cpu().numpy())):
        q = np.unique(q, axis=0)
        target = metrics._OffgridTarget(q, cloud.cpu().numpy(), p.device)
        ws = torch.empty(int(lib.pcgc_offgrid_workspace_bytes(target.res, len(q))), dtype=torch.uint8, device=p.device)
        fig, ts = timed(lambda: metrics._offgrid_mse(cloud, target, None, ws), repeats)
        line("pc_error_float, one direction: %s" % label, ts, "   %d target points, rms %.4f" % (len(q), np.sqrt(fig[0])))
    (_, _, report), ts = timed(lambda: surface.reconstruct(p, nr, bits, radius, simplify=2), repeats)
    line("surface.reconstruct(simplify=2)", ts)
    (_, _, report), ts = timed(lambda: surface.reconstruct(p, nr, bits, radius, simplify=2, error=True), repeats)
    line("surface.reconstruct(simplify=2, error=True)", ts)
    print("  " + surface.summary_line(report).replace("\n", "\n  "))


def scan_cloud(name, n_points, bits_, radius, repeats):
    points, _ = make_scan(n_points, 1)
    vox = voxels(points, bits_).contiguous()
    normals = metrics.estimate_normals(vox)
    print("%s: the scan of tools/register_bench.py, %d points, %d bits: %d occupied voxels; radius %d; %d repeats" % (
        name, len(points), bits_, len(vox), radius, repeats))
    return surface._validated(vox, normals, bits_)


def error_cloud(name, n_points, bits_, radius, repeats):
    """the mesh_error lines alone: the mesh built once, untimed"""
    p, nr, key, bits = scan_cloud(name, n_points, bits_, radius, repeats)
    spec = surface.parse_orient("propagate")
    lat = surface._Lattice(p, bits)
    seed, _ = surface._seeds(p, key, bits, spec.gap)
    sign, _, _ = lat.orient(nr, seed, spec.gap, surface.DEFAULT_TAU)
    lat.lattice()
    _, f = lat.implicit((sign.double()[:, None] * nr.double()).contiguous(), radius)
    v, t = lat.mesh(f, lat.triangle_ids(f))
    del lat, f
    sv, st, _ = surface._simplify_device(v, t, bits, 2)
    mesh_error_lines(p, nr, bits, radius, [("unsimplified", v, t), ("cell 2", sv, st)], repeats)


def one_cloud(name, n_points, bits_, radius, repeats):
    points, _ = make_scan(n_points, 1)
    vox = voxels(points, bits_).contiguous()
    out, ts = timed(lambda: metrics.estimate_normals(vox), 3, warmup=1)
    print("%s: the scan of tools/register_bench.py, %d points, %d bits: %d occupied voxels; radius %d; %d repeats" % (
        name, len(points), bits_, len(vox), radius, repeats))
    line("estimate_normals (not part of the call below)", ts)
    p, nr, key, bits = surface._validated(vox, out, bits_)
    spec, tau = surface.parse_orient("propagate"), surface.DEFAULT_TAU
    lat = surface._Lattice(p, bits)
    (seed, n_components), ts = timed(lambda: surface._seeds(p, key, bits, spec.gap), repeats)
    line("seeds: components, the largest key per label", ts, "   %d components" % n_components.item())
    for batch in (8, surface.ROUNDS_PER_READ, 256):
        (sign, rounds, reads), ts = timed(lambda: lat.orient(nr, seed, spec.gap, tau, batch), repeats)
        line("pcgc_surface_orient, %d rounds per read-back" % batch, ts, "   %d rounds, %d read-backs" % (rounds, reads))
    N = (sign.double()[:, None] * nr.double()).contiguous()
    (n_cells, n_lattice), ts = timed(lat.lattice, repeats)
    line("pcgc_surface_lattice (cells and vertices)", ts, "   %d cells, %d vertices" % (n_cells, n_lattice))
    (_, f), ts = timed(lambda: lat.implicit(N, radius), repeats)
    line("pcgc_surface_implicit, R = %d" % radius, ts)
    if radius != 5:
        line("pcgc_surface_implicit, R = 5", timed(lambda: lat.implicit(N, 5), repeats)[1])
    ids, ts = timed(lambda: lat.triangle_ids(f), repeats)
    line("pcgc_surface_triangles (count, read, emit)", ts, "   %d triangles" % len(ids))
    (v, t), ts = timed(lambda: lat.mesh(f, ids), repeats)
    line("torch.unique of the ids, pcgc_surface_mesh", ts, "   %d vertices" % len(v))
    # the parts of simplify at cell 2 on that mesh, as _simplify_device chains them
    tc, ts = timed(lambda: surface._canonical_device(t, len(v), surface.PACK_LIMIT), repeats)
    line("simplify: canonical order of the triangles", ts)
    s = surface._Simplifier(v, bits, 2)
    K, ts = timed(s.clusters, repeats)
    line("simplify: keys, unique, vertices by cluster", ts, "   %d clusters" % K)
    _, ts = timed(lambda: s.incidence(tc), repeats)
    line("simplify: incidence words, their stable sort", ts)
    _, ts = timed(lambda: s.place(tc), repeats)
    line("simplify: pcgc_simplify_place", ts)
    _, ts = timed(lambda: s.remap(tc), repeats)
    line("simplify: remap, unique, multiplicities", ts)
    (sv, st, _), ts = timed(lambda: surface._simplify_device(v, t, bits, 2), repeats)
    line("simplify: the whole of it on the device", ts, "   %d vertices, %d triangles" % (len(sv), len(st)))
    del ids, tc, s, lat, f
    mesh_error_lines(p, nr, bits, radius, [("unsimplified", v, t), ("cell 2", sv, st)], repeats)
    del v, t, sv, st
    (v, t, report), ts = timed(lambda: surface.reconstruct(p, nr, bits, radius), repeats)
    line("surface.reconstruct (normals given, mesh to the host)", ts)
    print("  " + surface.summary_line(report))
    (v, t, report), ts = timed(lambda: surface.reconstruct(p, nr, bits, radius, simplify=2), repeats)
    line("surface.reconstruct(simplify=2), the same session", ts)
    print("  " + surface.summary_line(report).replace("\n", "\n  "))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--radius", type=int, default=surface.DEFAULT_RADIUS)
    ap.add_argument("--no_rule", action="store_true", help="skip the numpy rule at 7 bits")
    ap.add_argument("--mesh_error_only", action="store_true", help="only the lines of metrics.mesh_error and its yardsticks, on both clouds")
    a = ap.parse_args()
    _lib.require_gpu()
    if a.mesh_error_only:
        error_cloud("sparse", 1000000, 10, a.radius, a.repeats)
        error_cloud("dense", 4000000, 9, a.radius, a.repeats)
        return
    one_cloud("sparse", 1000000, 10, a.radius, a.repeats)
    one_cloud("dense", 4000000, 9, a.radius, a.repeats)
    if a.no_rule:
        return
    import _surface_ref as ref
    ball = ref.sphere((63.5, 63.5, 63.5), 50.0, n=1500000)
    normals = metrics.estimate_normals(ball)
    t0 = time.perf_counter()
    want_v, want_t, _ = ref.reconstruct(ball, normals, 7, a.radius)
    dt = time.perf_counter() - t0
    (v, t, _), ts = timed(lambda: surface.reconstruct(ball, normals, 7, a.radius), a.repeats)
    same = v.tobytes() == want_v.tobytes() and np.array_equal(surface.canonical(t), surface.canonical(want_t))
    line("a sphere of %d voxels at 7 bits: surface.reconstruct" % len(ball), ts, "   the numpy rule (CPU, one call): %.2f s, %s" % (
        dt, "the same mesh" if same else "ANOTHER MESH"))


if __name__ == "__main__":
    main()
