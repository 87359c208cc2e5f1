"""Writing a mesh (mesh.write_triangle_mesh; csrc/slmeshwrite.inl) of the Poisson
mesh of a synthetic closed surface: a unit sphere of ``--points`` points with
outward normals, meshed at ``--depths`` and trimmed at the 0.02 quantile, and the
deepest mesh once more after simplify_vertex_clustering at 2 grid steps.

    python scripts/mesh_write_bench.py                      # depths 8, 10 + depth 10 simplified
    python scripts/mesh_write_bench.py --depths 8 --reps 5

Prints one JSON line per mesh: milliseconds (median of ``--reps`` after one
warm-up; wall time around blocking calls), bytes and GB/s, all in this process,
to files in one directory (``--dir``, default a temporary one) that are
overwritten every time, so the page cache is warm, of
  host_stl    the NumPy route of write_triangle_mesh (the writer before the
              device one) called with the mesh on the device: the copy back it
              needs, the NumPy passes and tofile;
  device_stl  the device route: packed on the GPU, streamed through the ring;
  device_ply  the same for the .ply (vertex normals included);
  pack_stl / pack_ply   the device routes with the file left out (packing and the
              copies into the pinned ring only);
and the host's share of the device routes (mesh.mesh_write_stats: waiting for
chunks to land, inside write()).  With ``--share`` (default on) it also times a
whole ``ProcessingLogic.reconstruct_stl`` call per depth on a binary PLY of the
cloud with its normals, once with the device writer and once with the host
route patched in, and prints the writer's share of each.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(fn, reps, stats=None):
    """-> (the median milliseconds of fn() over reps after one warm-up, the median of stats())."""
    import torch
    ms, rows = [], []
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if rep:
            ms.append((time.perf_counter() - t0) * 1e3)
            if stats:
                rows.append(stats())
    med = {k: round(statistics.median(r[k] for r in rows), 3) for k in rows[0]} if rows else {}
    return round(statistics.median(ms), 3), med


def gbps(n_bytes, ms):
    return round(n_bytes / (ms * 1e-3) / 1e9, 3)


def write_lines(name, V, T, d, reps):
    from structured_light_for_3d_model_replication_amd import mesh
    stl, ply = os.path.join(d, "bench.stl"), os.path.join(d, "bench.ply")
    out = {"mesh": name, "reps": reps, "vertices": len(V), "triangles": len(T)}
    ms, _ = timed(lambda: mesh.write_triangle_mesh(stl, V.cpu(), T.cpu()), reps)
    out["stl_bytes"] = os.path.getsize(stl)
    out["host_stl_ms"], out["host_stl_gbps"] = ms, gbps(out["stl_bytes"], ms)
    ms, st = timed(lambda: mesh.write_triangle_mesh(stl, V, T), reps, mesh.mesh_write_stats)
    assert os.path.getsize(stl) == out["stl_bytes"]
    out["device_stl_ms"], out["device_stl_gbps"] = ms, gbps(out["stl_bytes"], ms)
    out["device_stl_wait_ms"], out["device_stl_write_ms"] = st["wait_ms"], st["write_ms"]
    out["device_over_host_stl"] = round(out["device_stl_ms"] / out["host_stl_ms"], 4)
    ms, st = timed(lambda: mesh._write_device(None, ".stl", V, T), reps, mesh.mesh_write_stats)
    out["pack_stl_ms"], out["pack_stl_gbps"] = ms, gbps(out["stl_bytes"] - 84, ms)
    ms, st = timed(lambda: mesh.write_triangle_mesh(ply, V, T), reps, mesh.mesh_write_stats)
    out["ply_bytes"] = os.path.getsize(ply)
    out["device_ply_ms"], out["device_ply_gbps"] = ms, gbps(out["ply_bytes"], ms)
    out["device_ply_wait_ms"], out["device_ply_write_ms"] = st["wait_ms"], st["write_ms"]
    ms, st = timed(lambda: mesh._write_device(None, ".ply", V, T), reps, mesh.mesh_write_stats)
    out["pack_ply_ms"] = ms
    for p in (stl, ply):
        os.remove(p)
    return out


def share_line(src, depth, d, reps):
    """A whole reconstruct_stl call with the device writer and with the host route in its place."""
    import contextlib
    import io

    from structured_light_for_3d_model_replication_amd import mesh, processing
    dst = os.path.join(d, "recon.stl")
    device_route = mesh.write_triangle_mesh
    took = {}

    def writer(route):
        def call(path, V, T):
            import torch
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if route == "host":
                device_route(path, V.cpu(), T.cpu())
            else:
                device_route(path, V, T)
            took.setdefault(route, []).append((time.perf_counter() - t0) * 1e3)
        return call

    out = {"reconstruct_stl_depth": depth, "reps": reps}
    for route in ("device", "host"):
        mesh.write_triangle_mesh = writer(route)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                ms, _ = timed(lambda: processing.ProcessingLogic.reconstruct_stl(src, dst, params={"depth": depth}), reps)
        finally:
            mesh.write_triangle_mesh = device_route
        w = round(statistics.median(took[route][1:]), 3)
        out[f"{route}_call_ms"], out[f"{route}_writer_ms"], out[f"{route}_writer_share"] = ms, w, round(w / ms, 4)
    out["stl_bytes"] = os.path.getsize(dst)
    os.remove(dst)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--points", type=int, default=4_000_000)
    ap.add_argument("--depths", type=int, nargs="*", default=[8, 10])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    ap.add_argument("--no-share", dest="share", action="store_false", help="skip the whole reconstruct_stl calls")
    a = ap.parse_args()
    import numpy as np
    import torch

    from structured_light_for_3d_model_replication_amd import mesh, ply
    from tests import mesh_oracle as mo
    Ph, Nh = mo.sphere(a.points, (0.1, -0.2, 0.3))
    P, N = torch.from_numpy(Ph).cuda(), torch.from_numpy(Nh).cuda()
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        for depth in a.depths:
            V, T, dens = mesh.create_from_point_cloud_poisson(P, N, depth=depth)
            V, T = mesh.trim_by_density(V, T, dens, 0.02)
            del dens
            print(json.dumps(write_lines(f"depth_{depth}", V, T, d, a.reps)), flush=True)
            if depth == max(a.depths):
                h = float(mesh.box(P, depth)[1])
                V, T = mesh.simplify_vertex_clustering(V, T, 2.0 * h)
                print(json.dumps(write_lines(f"depth_{depth}_simplified_2h", V, T, d, a.reps)), flush=True)
            del V, T
        if a.share:
            src = os.path.join(d, "cloud.ply")
            ply.save_ply_open3d(Ph, np.zeros((len(Ph), 3), np.uint8), src, normals=Nh)
            for depth in a.depths:
                print(json.dumps(share_line(src, depth, d, a.reps)), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
