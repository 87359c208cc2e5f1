"""Per-edge cost of the loop-closing 360 merge on one GPU.

    python scripts/posegraph_bench.py [--sizes 1080p,4k] [--repeat 5] [--timeout 300]

Prints one JSON line per step.  Every step is a child process of its own under
``--timeout`` seconds; a step that fails or times out ends the run there.

Views are synthetic: a lumpy height field sampled on an H x W pixel grid at
0.25 units per pixel (1080p: 2.07 M points, 4K: 8.29 M), voxel size 1, so the
0.4-voxel ball of a correspondence search holds about eight points.  The
source is the same surface sampled half a pixel off and moved by a small rigid
motion, which the ICP has to undo.

Steps per size (wall time of the blocking call, median of ``--repeat`` after a
warm-up; the clouds are on the device beforehand):
  info     merge.get_information_matrix_from_point_clouds (k_info_fold)
  icp0     merge.registration_icp(max_iteration=0): one correspondence pass and
           one fold of the existing ICP kernels, the yardstick for ``info``
           (both build the target's search grid)
  icp      merge.registration_icp at 0.4 voxel, 30 iterations at most, and the
           target's normals (radius 2 voxel, max_nn 30) it needs
And once: ``optimise``: merge.global_optimization (host) on rings of 12 and 36
nodes with exact edges and 1 degree of drift per node.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SIZES = {"1080p": (1080, 1920), "4k": (2160, 3840)}
PITCH, VOXEL = 0.25, 1.0


def view(H, W, offset, device):
    import torch
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=device),
                          torch.arange(W, dtype=torch.float64, device=device), indexing="ij")
    x, y = (u + offset) * PITCH, (v + offset) * PITCH
    z = 20.0 * torch.sin(x / 37.0) * torch.cos(y / 23.0) + 5.0 * torch.sin(x / 5.0 + y / 7.0)
    return torch.stack([x.ravel(), y.ravel(), z.ravel()], dim=1).contiguous()


def small_motion():
    a = math.radians(0.05)
    M = np.eye(4)
    M[:3, :3] = [[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]]
    M[:3, 3] = [0.05, -0.04, 0.06]
    return M


def timed(fn, repeat, sync):
    fn()
    sync()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), out


def gpu_step(step, size, repeat):
    import torch
    from structured_light_for_3d_model_replication_amd import merge
    if not torch.cuda.is_available():
        raise RuntimeError("posegraph_bench needs a GPU")
    dev = torch.device("cuda", 0)
    H, W = SIZES[size]
    target = view(H, W, 0.0, dev)
    source = merge.transform(view(H, W, 0.5, dev), small_motion(), device=dev)
    d = 0.4 * VOXEL
    sync = torch.cuda.synchronize
    res = {"step": step, "size": size, "points": int(target.shape[0]), "max_distance": d, "repeat": repeat}
    if step == "info":
        med, best, (G, n) = timed(lambda: merge.get_information_matrix_from_point_clouds(
            source, target, d, np.eye(4), info=True, device=dev), repeat, sync)
        res.update(ms_median=med, ms_min=best, correspondences=n)
    else:
        t0 = time.perf_counter()
        normals = merge.estimate_normals(target, 2 * VOXEL, 30, device=dev)
        sync()
        res["normals_ms_first_call"] = (time.perf_counter() - t0) * 1e3
        iters = 0 if step == "icp0" else 30
        med, best, out = timed(lambda: merge.registration_icp(source, target, normals, d, np.eye(4),
                                                              max_iteration=iters, device=dev), repeat, sync)
        res.update(ms_median=med, ms_min=best, iterations=out["iterations"], fitness=out["fitness"],
                   inlier_rmse=out["inlier_rmse"])
    return res


def ring(n):
    from structured_light_for_3d_model_replication_amd import merge

    def pose(k, drift):
        a = 2.0 * math.pi * k / n + math.radians(drift * k)
        M = np.eye(4)
        M[:3, :3] = [[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]]
        M[:3, 3] = [100.0 * math.cos(a), 100.0 * math.sin(a), 0.1 * k * drift]
        return M
    truth = [pose(k, 0.0) for k in range(n)]
    info = np.diag([1e6, 1e6, 1e6, 1e3, 1e3, 1e3]).astype(np.float64)
    pairs = [(s, t) for s in range(n) for t in range(s + 1, n) if t == s + 1 or (s == 0 and t == n - 1)]
    edges = [(s, t, merge.mat4(merge.rigid_inverse(truth[t]), truth[s]), info, False) for s, t in pairs]
    return merge.PoseGraph([pose(k, 1.0) for k in range(n)], edges)


def optimise_step(repeat):
    from structured_light_for_3d_model_replication_amd import merge
    out = []
    for n in (12, 36):
        ts = []
        for _ in range(repeat + 1):
            g = ring(n)
            t0 = time.perf_counter()
            info = merge.global_optimization(g, max_correspondence_distance=0.4 * VOXEL)
            ts.append((time.perf_counter() - t0) * 1e3)
        out.append(dict(step="optimise", nodes=n, edges=len(g.edges), ms_median=statistics.median(ts[1:]),
                        ms_min=min(ts[1:]), **info))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1080p,4k")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--step", help="(internal) run one step in this process")
    ap.add_argument("--size")
    a = ap.parse_args()
    if a.step:
        rows = optimise_step(a.repeat) if a.step == "optimise" else [gpu_step(a.step, a.size, a.repeat)]
        for r in rows:
            print(json.dumps(r), flush=True)
        return 0
    steps = [("optimise", None)] + [(s, size) for size in a.sizes.split(",") for s in ("info", "icp0", "icp")]
    for step, size in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--repeat", str(a.repeat)]
        if size:
            cmd += ["--size", size]
        try:
            code = subprocess.run(cmd, timeout=a.timeout).returncode
        except subprocess.TimeoutExpired:
            code = 124
        if code != 0:  # nothing more is started on the GPU after a failed step
            print(json.dumps({"step": step, "size": size, "failed": code}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
