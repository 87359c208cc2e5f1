"""Mesh hole filling (mesh.fill_holes, boundary_loops; csrc/slmeshfill.inl) of the Poisson
mesh of a synthetic closed surface: a unit sphere of ``--points`` points with
outward normals, meshed at ``--depths`` and trimmed at the 0.02 quantile.

    python scripts/mesh_fill_bench.py                     # depths 6 (with the oracle), 8, 10 + reconstruct_stl at 10
    python scripts/mesh_fill_bench.py --depths 8 --reps 5 --e2e-depths

Prints one JSON line per depth: milliseconds (median of ``--reps`` after one
warm-up; wall time around blocking calls, the mesh on the device) of
``fill_holes`` -- two library calls, the first of which only counts -- with the
stages of the second (from sl_mesh_fill_stats), of ``boundary_loops``, and of
``is_watertight`` (one sl_mesh_check: it sorts the same 3 T side keys and is the
yardstick) in the same run; the counts of the fill; and what ``check`` says
before and after.  At ``--oracle-depth`` it also prints the time of the NumPy
restatement tests/meshfill_oracle.py on this host and the same mesh (NOT
Open3D, which is not installed) and whether the device results equal it.  At
``--e2e-depths`` a whole ProcessingLogic.reconstruct_stl call from a .ply to an
.stl is timed with and without ``fill_holes=True``.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SAID = ("boundary_edges", "non_manifold_edges", "inconsistent_edges", "non_manifold_vertices", "orientable",
        "watertight", "area", "volume")


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


def run(P, N, depth, reps):
    import torch

    from structured_light_for_3d_model_replication_amd import mesh
    V, T, d = mesh.create_from_point_cloud_poisson(P, N, depth=depth)
    V, T = mesh.trim_by_density(V, T, d, 0.02)
    del d
    out = {"depth": depth, "points": len(P), "reps": reps, "vertices": len(V), "triangles": len(T)}
    ms, res, st = timed(lambda: mesh.fill_holes(V, T, info=True), reps, mesh.fill_stats)
    out["fill_ms"] = ms
    out.update(st)
    out["second_call_ms"] = round(sum(st.values()), 3)
    out["sort_share_of_second_call"] = round(st["sort_ms"] / max(out["second_call_ms"], 1e-9), 3)
    out.update(res[2])
    Vf, Tf = res[0], res[1]
    ms, loops, _ = timed(lambda: mesh.boundary_loops(V, T), reps)
    out["boundary_loops_ms"] = ms
    out["largest_loop_sides"] = int(loops["size"].max()) if len(loops["size"]) else 0
    ms, _, st = timed(lambda: mesh.is_watertight(V, T), reps, mesh.check_stats)
    out["topology_ms"], out["topology_sort_ms"], out["topology_side_keys_ms"] = ms, st["sort_ms"], st["side_keys_ms"]
    out["fill_over_topology"] = round(out["fill_ms"] / ms, 3)
    before, after = mesh.check(V, T), mesh.check(Vf, Tf)
    out["before"] = {k: before[k] for k in SAID}
    out["after"] = {k: after[k] for k in SAID}
    out["peak_device_bytes"] = torch.cuda.max_memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    return out, V, T, (Vf, Tf, res[2])


def end_to_end(Ph, Nh, depth, reps):
    """A whole reconstruct_stl call, .ply to .stl, with and without fill_holes=True."""
    import numpy as np
    import torch

    from structured_light_for_3d_model_replication_amd import ply, processing
    out = {"depth": depth, "points": len(Ph), "reps": reps, "what": "reconstruct_stl"}
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "sphere.ply"), os.path.join(d, "sphere.stl")
        ply.save_ply_open3d(Ph, np.zeros((len(Ph), 3), np.uint8), src, normals=Nh)
        for name, kw in (("plain_ms", {}), ("fill_holes_ms", {"fill_holes": True})):
            ms = []
            for rep in range(reps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()) as text:
                    processing.ProcessingLogic.reconstruct_stl(src, dst, params={"depth": depth}, **kw)
                torch.cuda.synchronize()
                if rep:
                    ms.append((time.perf_counter() - t0) * 1e3)
            out[name] = round(statistics.median(ms), 1)
            out[name.replace("_ms", "_stl_bytes")] = os.path.getsize(dst)
            if kw:
                out["line"] = [x for x in text.getvalue().splitlines() if "Fill holes" in x][0]
    out["fill_holes_adds_ms"] = round(out["fill_holes_ms"] - out["plain_ms"], 1)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--points", type=int, default=4_000_000)
    ap.add_argument("--depths", type=int, nargs="*", default=[8, 10])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--oracle-depth", type=int, default=6, help="0: skip the NumPy oracle")
    ap.add_argument("--e2e-depths", type=int, nargs="*", default=[10])
    a = ap.parse_args()
    import numpy as np
    import torch

    from tests import mesh_oracle as mo
    from tests import meshfill_oracle as fo
    Ph, Nh = mo.sphere(a.points, (0.1, -0.2, 0.3))
    P, N = torch.from_numpy(Ph).cuda(), torch.from_numpy(Nh).cuda()
    if a.oracle_depth:
        line, V, T, got = run(P, N, a.oracle_depth, a.reps)
        t0 = time.perf_counter()
        wantV, wantT, want = fo.fill_holes(V.cpu().numpy(), T.cpu().numpy())
        line["oracle_fill_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        line["fill_equals_oracle"] = bool(np.array_equal(got[0].cpu().numpy(), wantV)
                                          and np.array_equal(got[1].cpu().numpy(), wantT) and got[2] == want)
        print(json.dumps(line), flush=True)
        del V, T, got
    for depth in a.depths:
        print(json.dumps(run(P, N, depth, a.reps)[0]), flush=True)
    del P, N
    for depth in a.e2e_depths:
        print(json.dumps(end_to_end(Ph, Nh, depth, a.reps)), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
