"""Mesh smoothing (mesh.adjacency_list, filter_smooth_laplacian,
filter_smooth_taubin; csrc/slmeshsmooth.inl) of the Poisson mesh of a synthetic
closed surface: a unit sphere of ``--points`` points with outward normals,
meshed at ``--depths`` and trimmed at the 0.02 quantile.

    python scripts/mesh_smooth_bench.py                     # depths 8, 10 + the oracle at depth 7
    python scripts/mesh_smooth_bench.py --depths 8 --reps 5 --e2e-depths

Prints one JSON line per depth: milliseconds (median of ``--reps`` after one
warm-up; wall time around blocking calls, the mesh on the device) of
adjacency_list with its stages (sl_mesh_smooth_stats), of ten Laplacian steps
and of ten Taubin iterations (the whole call, and the iteration stage alone per
step).  Every step is set against its traffic figure: the bytes of
``neighbours`` and ``row_start`` plus one read and one write of the vertices,
divided by the bandwidth the linear read / write kernel of
scripts/micro/step_floor (variant ``mix``) reaches on the same box, run first
(``--bandwidth-tbps`` to give it instead; without either the ratio is omitted).
At ``--e2e-depths`` a whole ProcessingLogic.reconstruct_stl call from a .ply to
an .stl is timed with and without ``smooth_iterations=10``.  At
``--oracle-depth`` it also prints the time of the NumPy restatement
tests/meshsmooth_oracle.py on this host and the same mesh (NOT Open3D, which is
not installed).
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
FLOOR = os.path.join(REPO, "scripts", "micro", "step_floor")


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


def floor_bandwidth():
    """TB/s moved by step_floor's ``mix`` variant (median of 3), or None when the binary is not built."""
    if not os.path.exists(FLOOR):
        return None
    out = subprocess.run([FLOOR, "--reps", "3", "--variants", "mix"], check=True, capture_output=True, text=True,
                         timeout=300).stdout
    rates = [json.loads(line)["moved_TBps"] for line in out.splitlines() if line.startswith("{")]
    return statistics.median(rates)


def run(P, N, depth, reps, tbps):
    import torch

    from structured_light_for_3d_model_replication_amd import mesh
    V, T, d = mesh.create_from_point_cloud_poisson(P, N, depth=depth)
    V, T = mesh.trim_by_density(V, T, d, 0.02)
    del d
    out = {"depth": depth, "points": len(P), "reps": reps, "vertices": len(V), "triangles": len(T)}
    ms, res, st = timed(lambda: mesh.adjacency_list(T, len(V), boundary=True), reps, mesh.smooth_stats)
    out["adjacency_ms"] = ms
    out.update({k: st[k] for k in ("keys_ms", "sort_ms", "csr_ms")})
    out["neighbours"] = len(res[1])
    out["boundary_vertices"] = int(res[2].sum())
    out["max_row"] = int((res[0][1:] - res[0][:-1]).max())
    del res
    step_bytes = 4 * out["neighbours"] + 8 * (len(V) + 1) + 2 * 24 * len(V)
    out["step_traffic_bytes"] = step_bytes
    if tbps:
        out["floor_tbps"] = tbps
        out["step_traffic_ms"] = round(step_bytes / (tbps * 1e12) * 1e3, 4)
    ms, _, st = timed(lambda: mesh.filter_smooth_laplacian(V, T, 10), reps, mesh.smooth_stats)
    out["laplacian_10_ms"] = ms
    out["laplacian_step_ms"] = round(st["iterations_ms"] / 10.0, 4)
    ms, _, st = timed(lambda: mesh.filter_smooth_taubin(V, T, 10), reps, mesh.smooth_stats)
    out["taubin_10_ms"] = ms
    out["taubin_10_iterations_ms"] = st["iterations_ms"]
    out["taubin_step_ms"] = round(st["iterations_ms"] / 20.0, 4)
    ms, _, st = timed(lambda: mesh.filter_smooth_simple(V, T, 10), reps, mesh.smooth_stats)
    out["simple_step_ms"] = round(st["iterations_ms"] / 10.0, 4)
    if tbps:
        for k in ("laplacian", "taubin", "simple"):
            out[f"{k}_step_over_traffic"] = round(out[f"{k}_step_ms"] / out["step_traffic_ms"], 2)
    out["peak_device_bytes"] = torch.cuda.max_memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    return out, V, T


def end_to_end(Ph, Nh, depth, reps):
    """A whole reconstruct_stl call, .ply to .stl, with and without ten Taubin iterations."""
    import numpy as np
    import torch

    from structured_light_for_3d_model_replication_amd import ply, processing
    out = {"depth": depth, "points": len(Ph), "reps": reps, "what": "reconstruct_stl"}
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "sphere.ply"), os.path.join(d, "sphere.stl")
        ply.save_ply_open3d(Ph, np.zeros((len(Ph), 3), np.uint8), src, normals=Nh)
        for name, kw in (("plain_ms", {}), ("taubin_10_ms", {"smooth_iterations": 10})):
            ms = []
            for rep in range(reps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    processing.ProcessingLogic.reconstruct_stl(src, dst, params={"depth": depth}, **kw)
                torch.cuda.synchronize()
                if rep:
                    ms.append((time.perf_counter() - t0) * 1e3)
            out[name] = round(statistics.median(ms), 1)
            out["stl_bytes"] = os.path.getsize(dst)
            os.remove(dst)
    out["smoothing_share"] = round(1.0 - out["plain_ms"] / out["taubin_10_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--points", type=int, default=4_000_000)
    ap.add_argument("--depths", type=int, nargs="*", default=[8, 10])
    ap.add_argument("--e2e-depths", type=int, nargs="*", default=[8, 10])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--oracle-depth", type=int, default=7, help="0: skip the NumPy oracle")
    ap.add_argument("--bandwidth-tbps", type=float, default=0.0, help="0: measure it with scripts/micro/step_floor")
    a = ap.parse_args()
    tbps = a.bandwidth_tbps or floor_bandwidth()  # (a child process of its own, before this one opens the device)
    import torch

    from tests import mesh_oracle as mo
    from tests import meshsmooth_oracle as so
    Ph, Nh = mo.sphere(a.points, (0.1, -0.2, 0.3))
    P, N = torch.from_numpy(Ph).cuda(), torch.from_numpy(Nh).cuda()
    if a.oracle_depth:
        line, V, T = run(P, N, a.oracle_depth, a.reps, tbps)
        Vh, Th = V.cpu().numpy(), T.cpu().numpy()
        t0 = time.perf_counter()
        so.adjacency_list(Th, len(Vh), boundary=True)
        line["oracle_adjacency_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        t0 = time.perf_counter()
        want = so.filter_smooth_taubin(Vh, Th, 10)
        line["oracle_taubin_10_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        from structured_light_for_3d_model_replication_amd import mesh
        line["equals_oracle"] = bool((mesh.filter_smooth_taubin(V, T, 10).cpu().numpy() == want).all())
        print(json.dumps(line), flush=True)
        del V, T
    for depth in a.depths:
        print(json.dumps(run(P, N, depth, a.reps, tbps)[0]), flush=True)
    del P, N
    for depth in a.e2e_depths:
        print(json.dumps(end_to_end(Ph, Nh, depth, a.reps)), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
