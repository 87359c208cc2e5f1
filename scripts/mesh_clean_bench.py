"""Mesh clean-up (mesh.cluster_connected_triangles, select_components,
simplify_vertex_clustering; csrc/slmeshclean.inl) of the Poisson mesh of a
synthetic closed surface: a unit sphere of ``--points`` points with outward
normals, meshed at ``--depths`` and trimmed at the 0.02 quantile.

    python scripts/mesh_clean_bench.py                     # depths 8, 10 + the oracle at depth 7
    python scripts/mesh_clean_bench.py --depths 8 --reps 5

Prints one JSON line per depth: milliseconds (median of ``--reps`` after one
warm-up; wall time around blocking calls, the mesh on the device) of
cluster_connected_triangles with and without areas, its stages (from
sl_mesh_cluster_triangles_stats; ``sort_ms`` is the radix sort of the 3 T edge
keys alone, on those keys, in the same run, and ``sort_share`` its share of the
call without areas), select_components(keep_largest=True) and
simplify_vertex_clustering at 2, 4 and 8 grid steps with the triangles and STL
bytes before and after.  At ``--oracle-depth`` it also prints the time of the
NumPy restatement tests/meshclean_oracle.py on this host and the same mesh (NOT
Open3D, which is not installed).
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

STAGES = ("edge_keys_ms", "sort_ms", "union_ms", "flatten_rank_ms", "counts_ms", "areas_ms")


def timed(fn, reps, stats=None):
    """-> (the median milliseconds of fn() over reps after one warm-up, the last result, the median of stats())."""
    import torch
    ms, rows, out = [], [], None
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if rep:
            ms.append((time.perf_counter() - t0) * 1e3)
            if stats:
                rows.append(stats())
    med = {k: round(statistics.median(r[k] for r in rows), 3) for k in rows[0]} if rows else {}
    return round(statistics.median(ms), 3), out, med


def stl_bytes(n_triangles):
    return 84 + 50 * int(n_triangles)


def run(P, N, depth, reps):
    import torch

    from structured_light_for_3d_model_replication_amd import mesh
    V, T, d = mesh.create_from_point_cloud_poisson(P, N, depth=depth)
    h = float(mesh.box(P, depth)[1])
    V, T = mesh.trim_by_density(V, T, d, 0.02)
    del d
    out = {"depth": depth, "points": len(P), "reps": reps, "vertices": len(V), "triangles": len(T),
           "stl_bytes": stl_bytes(len(T))}
    ms, res, st = timed(lambda: mesh.cluster_connected_triangles(V, T, area=False), reps, mesh.cluster_stats)
    out["cluster_ms"] = ms
    out.update(st)
    out.pop("areas_ms")
    out["clusters"] = len(res[1])
    out["largest_cluster"] = int(res[1].max())
    out["sort_share"] = round(st["sort_ms"] / ms, 3)
    out["union_flatten_rank_over_sort"] = round((st["union_ms"] + st["flatten_rank_ms"]) / st["sort_ms"], 3)
    ms, res, st = timed(lambda: mesh.cluster_connected_triangles(V, T), reps, mesh.cluster_stats)
    out["cluster_with_areas_ms"] = ms
    out["areas_ms"] = st["areas_ms"]
    out["largest_area"] = float(res[2].max())
    ms, res, _ = timed(lambda: mesh.select_components(V, T, keep_largest=True), reps)
    out["select_largest_ms"] = ms
    out["select_largest_triangles"] = len(res[1])
    del res
    for steps in (2, 4, 8):
        ms, res, _ = timed(lambda: mesh.simplify_vertex_clustering(V, T, steps * h), reps)
        out[f"simplify_{steps}h_ms"] = ms
        out[f"simplify_{steps}h_vertices"] = len(res[0])
        out[f"simplify_{steps}h_triangles"] = len(res[1])
        out[f"simplify_{steps}h_stl_bytes"] = stl_bytes(len(res[1]))
        del res
    out["peak_device_bytes"] = torch.cuda.max_memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    return out, V, T, h


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--points", type=int, default=4_000_000)
    ap.add_argument("--depths", type=int, nargs="*", default=[8, 10])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--oracle-depth", type=int, default=7, help="0: skip the NumPy oracle")
    a = ap.parse_args()
    import torch

    from tests import mesh_oracle as mo
    from tests import meshclean_oracle as oc
    Ph, Nh = mo.sphere(a.points, (0.1, -0.2, 0.3))
    P, N = torch.from_numpy(Ph).cuda(), torch.from_numpy(Nh).cuda()
    if a.oracle_depth:
        line, V, T, h = run(P, N, a.oracle_depth, a.reps)
        Vh, Th = V.cpu().numpy(), T.cpu().numpy()
        t0 = time.perf_counter()
        oc.cluster_connected_triangles(Th, len(Vh), Vh)
        line["oracle_cluster_with_areas_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        t0 = time.perf_counter()
        oc.simplify_vertex_clustering(Vh, Th, 2 * h)
        line["oracle_simplify_2h_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        print(json.dumps(line), flush=True)
        del V, T
    for depth in a.depths:
        print(json.dumps(run(P, N, depth, a.reps)[0]), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
