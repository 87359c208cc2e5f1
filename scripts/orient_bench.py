"""Consistent tangent-plane normal orientation (mesh.orient_normals_consistent_
tangent_plane, csrc/slorient.inl) of a synthetic surface that the radial
orientation gets wrong: a torus (R = 1, r = 0.4) of ``--points`` points -- the
size of the merged cloud scripts/merge_bench.py ends with -- whose analytic
normals carry random signs.

    python scripts/orient_bench.py                   # k = 30 and 100 + the oracle at 800 000 points
    python scripts/orient_bench.py --points 500000 --ks 12 --reps 5

Prints one JSON line per k: milliseconds of the two stages, ``radius_search``
(the graph) and the orientation on that graph (median of ``--reps`` after one
warm-up; wall time around blocking calls with the device synchronised), the
Boruvka rounds and the pointer-jump launches of each round, the components and
the share of normals that come out on the outward side.  ``--radius`` defaults
to the one that holds about 150 points, so k = 100 cuts most rows.  At
``--oracle-points`` it also prints the time of the only CPU baseline there is
here, the NumPy/Python restatement tests/orient_oracle.py, on this host and on
the GPU's graph (NOT Open3D, which is not installed).
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

AREA = 4.0 * np.pi ** 2 * 1.0 * 0.4  # of the torus


def cloud(n, seed=0):
    from tests import orient_oracle as oo
    P, out = oo.torus(n, seed)
    sign = np.random.default_rng(seed + 100).choice([-1.0, 1.0], size=(n, 1))
    return P, out, out * sign


def run(P, N, out, radius, k, reps):
    import torch

    from structured_light_for_3d_model_replication_amd import merge, mesh
    ts, to = [], []
    for rep in range(reps + 1):  # the first is the warm-up: code objects, the scratch pool
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        idx, _, cnt = merge.radius_search(P, radius, k)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        got, info = mesh.orient_normals_mst(P, N, idx, cnt)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if rep:
            ts.append((t1 - t0) * 1e3)
            to.append((t2 - t1) * 1e3)
    line = {"points": len(P), "k": k, "radius": round(radius, 6), "reps": reps,
            "mean_neighbours": round(float(cnt.double().mean()), 2),
            "radius_search_ms": round(statistics.median(ts), 3), "orient_ms": round(statistics.median(to), 3),
            "rounds": info["rounds"], "jump_launches": info["jumps"], "components": info["components"],
            "tree_edges": len(info["tree_slots"]),
            "outward_share": round(float(((got * out).sum(1) > 0).double().mean()), 6)}
    return line, (idx, cnt, got)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--points", type=int, default=3_400_000)
    ap.add_argument("--ks", type=int, nargs="*", default=[30, 100])
    ap.add_argument("--radius", type=float, default=0.0, help="0: the radius that holds about 150 points")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--oracle-points", type=int, default=800_000, help="0: skip the NumPy oracle")
    ap.add_argument("--oracle-k", type=int, default=30)
    a = ap.parse_args()
    import torch

    from tests import orient_oracle as oo

    def radius_for(n):
        return a.radius or float(np.sqrt(150.0 * AREA / (np.pi * n)))

    if a.oracle_points:
        Ph, outh, Nh = cloud(a.oracle_points)
        P, N, out = (torch.from_numpy(x).cuda() for x in (Ph, Nh, outh))
        line, (idx, cnt, got) = run(P, N, out, radius_for(a.oracle_points), a.oracle_k, a.reps)
        idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
        t0 = time.perf_counter()
        exp, tree, comps = oo.orient(Ph, Nh, idx, cnt)
        line["oracle_numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        line["oracle_equal"] = bool(np.array_equal(got.cpu().numpy(), exp) and comps == line["components"])
        print(json.dumps(line), flush=True)
        del P, N, out, idx, cnt, got
    Ph, outh, Nh = cloud(a.points)
    P, N, out = (torch.from_numpy(x).cuda() for x in (Ph, Nh, outh))
    for k in a.ks:
        print(json.dumps(run(P, N, out, radius_for(a.points), k, a.reps)[0]), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
