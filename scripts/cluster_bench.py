"""Density clustering of one view (merge.cluster_dbscan and its companions,
csrc/slcluster.inl) at the reference's own parameters -- Old/
StatisticalOutlierRemoval.py: cluster_dbscan(eps=5, min_points=200), then
remove_radius_outlier(nb_points=5, radius=15) -- on a synthetic turntable view
in millimetres: an object (a hemisphere of radius 80 facing the camera), the
wall behind it (500 x 360) and a detached clump (a sphere of radius 15), depth
noise 0.2, points in random order.

    python scripts/cluster_bench.py                       # a 1080p-sized and a 4K-sized view + the oracle
    python scripts/cluster_bench.py --points 500000 --reps 5 --oracle-points 0

Prints one JSON line per size: the points per eps-ball (mean exact count), the
milliseconds of sl_cluster_dbscan's stages (grid, count, union, flatten + rank,
border: host clock around a stream synchronisation per stage) and of the whole
call, of the radius filter, of the nearest-neighbour distance and of the recipe
(median of ``--reps`` after one warm-up, wall time around blocking calls), the
clusters and the size of the largest.  At ``--oracle-points`` (the same scene
with every length shrunk so that an eps-ball holds about as many points as at 1 M) it also
prints the time of the only CPU baseline there is here, the NumPy/SciPy
restatement tests/cluster_oracle.py, on this host (NOT Open3D, which is not
installed), and whether the labels are equal.
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

EPS, MIN_POINTS, NB_POINTS, RADIUS = 5.0, 200, 5, 15.0


def view(n, scale=1.0, seed=0):
    """n points: 45 % object, 50 % wall, 5 % clump; every length times ``scale``."""
    rng = np.random.default_rng(seed)
    n_obj, n_clump = int(0.45 * n), int(0.05 * n)
    n_wall = n - n_obj - n_clump

    def sphere(m, radius, centre, front_only):
        v = rng.normal(size=(m, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        if front_only:
            v[:, 2] = -np.abs(v[:, 2])
        return v * radius + centre
    obj = sphere(n_obj, 80.0, np.array([0.0, 0.0, 500.0]), True)
    wall = np.stack([rng.uniform(-250, 250, n_wall), rng.uniform(-180, 180, n_wall), np.full(n_wall, 700.0)], 1)
    clump = sphere(n_clump, 15.0, np.array([150.0, 100.0, 450.0]), False)
    P = np.concatenate([obj, wall, clump])
    P[:, 2] += rng.normal(size=n) * 0.2
    return np.ascontiguousarray(P[rng.permutation(n)] * scale)


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


def run(Ph, reps):
    import torch

    from structured_light_for_3d_model_replication_amd import merge
    P = torch.from_numpy(Ph).cuda()
    eps, radius = EPS, RADIUS
    stages = []

    def dbscan():
        out = merge.cluster_dbscan(P, eps, MIN_POINTS, info=False)
        stages.append(merge.cluster_dbscan_stage_ms())
        return out
    dbscan_ms, labels = timed(dbscan, reps)
    stage_ms = {k: round(statistics.median(s[k] for s in stages[1:]), 3) for k in stages[0]}
    exact_ms, cnt = timed(lambda: merge.radius_count(P, eps), 1)
    radius_ms, ind = timed(lambda: merge.remove_radius_outlier(P, NB_POINTS, radius), reps)
    nn_ms, _ = timed(lambda: merge.compute_nearest_neighbor_distance(P), reps)

    def recipe():
        merge.compute_nearest_neighbor_distance(P)
        Q, _ = merge.keep_largest_cluster(P, None, eps, MIN_POINTS)
        return merge.select_by_index(Q, None, merge.remove_radius_outlier(Q, NB_POINTS, radius))[0]
    recipe_ms, kept = timed(recipe, reps)
    sizes = torch.bincount(labels[labels >= 0].long())
    line = {"points": len(Ph), "eps": eps, "min_points": MIN_POINTS, "reps": reps,
            "mean_ball": round(float(cnt.double().mean()), 1), "max_ball": int(cnt.max()),
            "stage_ms": stage_ms, "dbscan_ms": dbscan_ms, "exact_count_ms": exact_ms,
            "radius_outlier_ms": radius_ms, "radius_kept": len(ind), "nn_distance_ms": nn_ms,
            "recipe_ms": recipe_ms, "recipe_kept": len(kept), "clusters": len(sizes),
            "largest": int(sizes.max()) if len(sizes) else 0, "noise": int((labels < 0).sum())}
    return line, labels


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--points", type=int, nargs="*", default=[1_000_000, 4_000_000],
                    help="a 1080p-sized and a 4K-sized view")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--oracle-points", type=int, default=40_000, help="0: skip the NumPy/SciPy oracle")
    a = ap.parse_args()
    if a.oracle_points:
        from tests import cluster_oracle as co
        scale = float(np.sqrt(a.oracle_points / 1_000_000))  # an eps-ball holds what it holds at 1 M points
        Ph = view(a.oracle_points, scale)
        line, labels = run(Ph, a.reps)
        t0 = time.perf_counter()
        want, info = co.dbscan_order_free(Ph, EPS, MIN_POINTS)
        line["oracle_numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        line["oracle_equal"] = bool(np.array_equal(labels.cpu().numpy(), want) and info["clusters"] == line["clusters"])
        print(json.dumps(line), flush=True)
    for n in a.points:
        print(json.dumps(run(view(n), a.reps)[0]), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
