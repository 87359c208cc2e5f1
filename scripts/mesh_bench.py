"""Poisson meshing (mesh.create_from_point_cloud_poisson, csrc/slmesh.inl) of a
synthetic closed surface: a unit sphere of ``--points`` points with outward
normals.

    python scripts/mesh_bench.py                     # depths 8, 9, 10 + the oracle at depth 7
    python scripts/mesh_bench.py --depths 8 --reps 5

Prints one JSON line per depth: milliseconds per stage (median of ``--reps``
after one warm-up; wall time around blocking calls with the device
synchronised), the 0.02-quantile trim, the mesh's size and the peak device
memory torch saw.  At ``--oracle-depth`` it also prints the time of the only
CPU baseline there is here, the NumPy restatement tests/mesh_oracle.py, on
this host and on the same points (NOT Open3D, which is not installed).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

STAGES = ("splat", "divergence", "solve", "iso", "extract", "density", "trim")


def run(P, N, depth, reps):
    import torch

    from structured_light_for_3d_model_replication_amd import mesh
    rows = []
    for rep in range(reps + 1):  # the first is the warm-up: code objects, rocFFT plans, the allocator's cache
        t = {}
        t0 = time.perf_counter()
        V, T, d = mesh.create_from_point_cloud_poisson(P, N, depth=depth, timings=t)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        V2, T2 = mesh.trim_by_density(V, T, d, 0.02)
        torch.cuda.synchronize()
        t["trim"] = (time.perf_counter() - t1) * 1e3
        t["total"] = (time.perf_counter() - t0) * 1e3
        if rep:
            rows.append(t)
        size = {"vertices": len(V), "triangles": len(T), "trimmed_vertices": len(V2), "trimmed_triangles": len(T2)}
        del V, T, d, V2, T2
    out = {"depth": depth, "points": len(P), "reps": reps}
    out.update({f"{k}_ms": round(statistics.median(r[k] for r in rows), 3) for k in STAGES + ("total",)})
    out.update(size)
    out["peak_device_bytes"] = torch.cuda.max_memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--points", type=int, default=4_000_000)
    ap.add_argument("--depths", type=int, nargs="*", default=[8, 9, 10])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--oracle-depth", type=int, default=7, help="0: skip the NumPy oracle")
    a = ap.parse_args()
    import torch

    from tests import mesh_oracle as mo
    Ph, Nh = mo.sphere(a.points, (0.1, -0.2, 0.3))
    P, N = torch.from_numpy(Ph).cuda(), torch.from_numpy(Nh).cuda()
    if a.oracle_depth:
        line = run(P, N, a.oracle_depth, a.reps)
        t0 = time.perf_counter()
        o = mo.poisson(Ph, Nh, a.oracle_depth)
        line["oracle_numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        line["oracle_triangles"] = len(o["triangles"])
        print(json.dumps(line), flush=True)
    for depth in a.depths:
        print(json.dumps(run(P, N, depth, a.reps)), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
