"""Ball-pivoting surface meshing of one view (mesh.create_from_point_cloud_
ball_pivoting, csrc/slbpa.inl) at the reference's own parameters --
server/processing.py:220-237: radii of 1, 2 and 4 times the mean
nearest-neighbour distance -- on a synthetic turntable view in millimetres: an
object (a hemisphere of radius 80 facing the camera) in front of a wall
(500 x 360), depth noise of a tenth of the point spacing, analytic normals
towards the camera, points in random order.

    python scripts/ball_pivoting_bench.py                       # a 1080p-sized and a 4K-sized view + the oracle
    python scripts/ball_pivoting_bench.py --points 500000 --reps 3 --oracle-points 0

Prints one JSON line per size: the radii, per radius the passes, the live
queries of each pass (the points that are not inner) and how many of them the
kernel's second tier took (a neighbourhood above 256 points), the milliseconds of the
passes (wall time around a device synchronisation) and of their enumerations
(grid + kernel + ordering, sl_ball_pivot_candidates_stats), the milliseconds of
the whole call and of the nearest-neighbour distance (median of ``--reps`` after
one warm-up), the triangles, the share of border edges among the mesh's edges
and the triangles the per-edge rule dropped.  At ``--oracle-points`` it also
prints the time of the only CPU baseline there is here, the NumPy/SciPy
restatement tests/bpa_oracle.py, on this host (NOT Open3D, which is not
installed), and whether the triangles are equal.
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

MULTIPLIERS = (1.0, 2.0, 4.0)


def view(n, seed=0):
    """n points and their normals: 20 % object, 80 % wall (about equal density)."""
    rng = np.random.default_rng(seed)
    n_obj = int(0.2 * n)
    n_wall = n - n_obj
    v = rng.normal(size=(n_obj, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v[:, 2] = -np.abs(v[:, 2])
    obj = v * 80.0 + np.array([0.0, 0.0, 500.0])
    wall = np.stack([rng.uniform(-250, 250, n_wall), rng.uniform(-180, 180, n_wall), np.full(n_wall, 700.0)], 1)
    P = np.concatenate([obj, wall])
    N = np.concatenate([v, np.tile([[0.0, 0.0, -1.0]], (n_wall, 1))])
    spacing = np.sqrt((2 * np.pi * 80.0 ** 2 + 500.0 * 360.0) / n)
    P += N * (rng.normal(size=(n, 1)) * 0.1 * spacing)
    perm = rng.permutation(n)
    return np.ascontiguousarray(P[perm]), np.ascontiguousarray(N[perm])


def timed(fn, reps):
    import torch
    ts, out = [], None
    for rep in range(reps + 1):  # the first is the warm-up: code objects, the scratch pool
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if rep:
            ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3), out


def run(Ph, Nh, reps):
    import torch

    from structured_light_for_3d_model_replication_amd import merge, mesh
    P, N = torch.from_numpy(Ph).cuda(), torch.from_numpy(Nh).cuda()
    nn_ms, d = timed(lambda: merge.compute_nearest_neighbor_distance(P), reps)
    avg = mesh.ordered_sum(d) / float(len(Ph))
    radii = [avg * m for m in MULTIPLIERS]
    runs = []

    def bpa():
        runs.append({})
        return mesh.create_from_point_cloud_ball_pivoting(P, N, radii, info=True, timings=runs[-1])
    total_ms, (_, T, info) = timed(bpa, reps)
    tm = runs[-1]
    per_radius, at = [], 0
    for r, passes in zip(radii, info["passes"]):
        sl = slice(at, at + passes)
        at += passes
        per_radius.append({"radius": round(r, 5), "passes": passes, "live": tm["live"][sl],
                           "second_tier": tm["second_tier"][sl], "triangles": info["triangles"][sl],
                           "dropped": info["dropped"][sl],
                           "pass_ms": [round(v, 2) for v in tm["ms"][sl]],
                           "grid_ms": [round(v, 2) for v in tm["grid_ms"][sl]],
                           "enumerate_ms": [round(v, 2) for v in tm["enumerate_ms"][sl]],
                           "order_ms": [round(v, 2) for v in tm["order_ms"][sl]]})
    edges = (3 * len(T) + info["border_edges"]) // 2
    line = {"points": len(Ph), "reps": reps, "mean_nn": round(avg, 5), "radii": per_radius, "total_ms": total_ms,
            "nn_distance_ms": nn_ms, "triangles": len(T), "edges": edges, "border_edges": info["border_edges"],
            "border_share": round(info["border_edges"] / max(edges, 1), 4), "converged": info["converged"]}
    return line, T, radii


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--points", type=int, nargs="*", default=[1_000_000, 4_000_000],
                    help="a 1080p-sized and a 4K-sized view")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--oracle-points", type=int, default=10_000, help="0: skip the NumPy/SciPy oracle")
    a = ap.parse_args()
    if a.oracle_points:
        from tests import bpa_oracle as bo
        Ph, Nh = view(a.oracle_points)
        line, T, radii = run(Ph, Nh, a.reps)
        t0 = time.perf_counter()
        want, _ = bo.ball_pivoting(Ph, Nh, radii)
        line["oracle_numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        line["oracle_equal"] = bool(np.array_equal(T.cpu().numpy(), want))
        print(json.dumps(line), flush=True)
    for n in a.points:
        print(json.dumps(run(*view(n), a.reps)[0]), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
