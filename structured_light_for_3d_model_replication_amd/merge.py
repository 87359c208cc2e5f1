"""Merge stage on the GPU (server/processing.py:116-182).

``merge_pro_360`` concatenates the per-view clouds in a common frame, then
``voxel_down_sample`` (:171) and ``remove_statistical_outlier(20, 2.0)`` +
``select_by_index`` (:174-175), and writes the result.  These are Open3D calls in
the reference.  Here they are HIP kernels of libslgpu.so (csrc/slmerge.hip)
with Open3D's arithmetic: same voxel grid, sums in point order, exact kNN, and
sequential cloud statistics.  Voxel output is in ascending voxel key rather than
Open3D's hash order.

Then ``estimate_normals(KDTreeSearchParamHybrid(radius=2 voxel, max_nn=30))``
(:178) and ``write_point_cloud`` (:181).  Open3D is not in this image, so
parity is unpinned; oracle/merge_oracle.py is the restatement the tests check
against.

Registration.  The reference aligns consecutive views by FPFH + RANSAC
(a global estimate) refined by point-to-plane ICP (:145-157) and accumulates
the transforms (:159-167).  ``merge_pro_360`` keeps that flow on the GPU:
``compute_fpfh_feature`` (sl_compute_fpfh), ``registration_ransac_based_on_
feature_matching`` (sl_ransac_feature_matching) and ``registration_icp``
(sl_icp_point_to_plane) -- Open3D's algorithms; parity vs Open3D unpinned,
oracle/registration_oracle.py and oracle/merge_oracle.py restate them.  With
``seed_poses`` (a turntable's known poses) the RANSAC estimate is replaced by
the relative pose between the two views.
``merge_pro_360_posed`` skips registration and takes the poses as they are
(the same ones ``Reconstructor.decode_triangulate`` applies inside k_cloud).

Closing the loop.  ``merge_360_pose_graph`` is the reference's full-turn
script (Old/new360Merge.py): neighbouring views and the pair (first, last)
registered on the full clouds (``full_registration``), each edge weighted by
``get_information_matrix_from_point_clouds`` (sl_information_matrix,
csrc/slinfo.inl) and the pose graph optimised by ``global_optimization``
(sl_pose_graph_optimize, host code, csrc/slposegraph.inl).  Parity vs Open3D
unpinned; tests/posegraph_oracle.py restates both.

Clean-up before the merge.  ``segment_plane`` (sl_segment_plane,
csrc/slplane.inl) is the plane RANSAC of ``remove_background``
(processing.py:25-52); ``processing.py`` of this package is the drop-in for the
reference's ``ProcessingLogic`` built on it.  Parity vs Open3D unpinned;
tests/plane_oracle.py restates it.
"""
from __future__ import annotations

import ctypes
import glob
import os
import re
import threading

import numpy as np
import torch

from . import _lib, core, ply

_engines: dict = {}
_engines_lock = threading.Lock()


def _engine(device) -> core.Reconstructor:
    dev = torch.device(device if device is not None else "cuda")
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    with _engines_lock:
        if idx not in _engines:
            _engines[idx] = core.Reconstructor(torch.device("cuda", idx))
        return _engines[idx]


def _read_cloud(path, dev):
    """ply.read_ply of a view's file, parsed on the device (ply.read_cloud_device) -> (points f64 [N,3],
    colours BGR u8 [N,3], zeros when the file has none)."""
    cloud = ply.read_cloud_device(path, device=dev)
    P, C = cloud["points"], cloud["colors"]
    return P, (C if C is not None else torch.zeros((len(P), 3), dtype=torch.uint8, device=dev))


def _call(eng, name, *args):
    """One libslgpu entry point of the (ctx, ..., stream) shape, under the engine's lock, checked."""
    with eng._lock:
        _lib.check(getattr(eng._L, name)(eng._ctx, *args, eng._stream(None)), eng._ctx, name)


def _f64(points, dev) -> torch.Tensor:
    P = torch.as_tensor(points)
    if P.dim() != 2 or P.shape[1] != 3:
        raise ValueError("points must be (N, 3)")
    return P.to(device=dev, dtype=torch.float64).contiguous()


def _u8(colors, dev, n) -> torch.Tensor | None:
    if colors is None:
        return None
    C = torch.as_tensor(colors).to(device=dev, dtype=torch.uint8).contiguous()
    if C.shape != (n, 3):
        raise ValueError("colors must be (N, 3) uint8")
    return C


def _ptr(t):
    return None if t is None else t.data_ptr()


def voxel_down_sample(points, colors=None, voxel_size: float = 0.02, *, device=None):
    """PointCloud.voxel_down_sample -> (points f64 [M,3], colors u8 [M,3] | None) on the device."""
    eng = _engine(device)
    P = _f64(points, eng.device)
    n = P.shape[0]
    C = _u8(colors, eng.device, n)
    out = torch.empty((max(n, 1), 3), dtype=torch.float64, device=eng.device)
    oc = None if C is None else torch.empty((max(n, 1), 3), dtype=torch.uint8, device=eng.device)
    m = ctypes.c_int64()
    _call(eng, "sl_voxel_downsample", _ptr(P), _ptr(C), n, float(voxel_size), out.data_ptr(), _ptr(oc), ctypes.byref(m))
    k = m.value
    return out[:k], (None if oc is None else oc[:k])


def remove_statistical_outlier(points, nb_neighbors: int = 20, std_ratio: float = 2.0, *, device=None):
    """PointCloud.remove_statistical_outlier -> (ind int64 [K] ascending, mean kNN distance f64 [N])."""
    eng = _engine(device)
    P = _f64(points, eng.device)
    n = P.shape[0]
    avg = torch.empty(max(n, 1), dtype=torch.float64, device=eng.device)
    ind = torch.empty(max(n, 1), dtype=torch.int64, device=eng.device)
    k = ctypes.c_int64()
    _call(eng, "sl_statistical_outliers", _ptr(P), n, int(nb_neighbors), float(std_ratio), avg.data_ptr(),
          ind.data_ptr(), ctypes.byref(k))
    return ind[: k.value], avg[:n]


def select_by_index(points, colors, ind, invert: bool = False, *, device=None):
    """PointCloud.select_by_index(ind, invert) -> (points, colors | None) on the
    device; ``invert=True`` selects the points ``ind`` does not list, in their
    original order."""
    eng = _engine(device)
    P = _f64(points, eng.device)
    C = _u8(colors, eng.device, P.shape[0])
    I = torch.as_tensor(ind).to(device=eng.device, dtype=torch.int64).contiguous()
    if I.shape[0] and (int(I.min()) < 0 or int(I.max()) >= P.shape[0]):
        raise IndexError("index out of range")
    if invert:  # the complement's index list (sl_index_complement); the gather below is the same kernel
        n = P.shape[0]
        rest = torch.empty(max(n, 1), dtype=torch.int64, device=eng.device)
        k = ctypes.c_int64()
        _call(eng, "sl_index_complement", I.data_ptr() if I.shape[0] else None, I.shape[0], n, rest.data_ptr(),
              ctypes.byref(k))
        I = rest[: k.value]
    m = I.shape[0]
    out = torch.empty((max(m, 1), 3), dtype=torch.float64, device=eng.device)
    oc = None if C is None else torch.empty((max(m, 1), 3), dtype=torch.uint8, device=eng.device)
    _call(eng, "sl_select_by_index", _ptr(P), _ptr(C), I.data_ptr(), m, out.data_ptr(), _ptr(oc))
    return out[:m], (None if oc is None else oc[:m])


def segment_plane(points, distance_threshold, ransac_n: int = 3, num_iterations: int = 100,
                  probability: float = 0.99999999, *, seed: int = 0, batch: int = 0, device=None):
    """PointCloud.segment_plane(distance_threshold, ransac_n, num_iterations,
    probability) (processing.py:37-39; Open3D's defaults) on the GPU
    (sl_segment_plane) -> (plane_model numpy [4], inliers int64 [K] ascending on
    the device, info).  ``info``: ``iterations`` (RANSAC iterations run before
    the early exit) and ``rest`` (the other points' indices, ascending, on the
    device: what ``select_by_index(inliers, invert=True)`` selects).

    Open3D's algorithm restated; parity with Open3D is unpinned (not in this
    image) and tests/plane_oracle.py is the bit-identical CPU restatement.  Two
    documented deviations: ``seed`` fixes a splitmix64 draw that may repeat a
    point within a sample (Open3D samples without replacement), and a cloud on
    which no hypothesis has an inlier returns the zero plane and no inliers.
    ``batch`` (hypotheses per GPU pass; 0: the default, 64) does not
    change the result."""
    eng = _engine(device)
    P = _f64(points, eng.device)
    n = P.shape[0]
    inl = torch.empty(max(n, 1), dtype=torch.int64, device=eng.device)
    rest = torch.empty(max(n, 1), dtype=torch.int64, device=eng.device)
    plane = np.zeros(4)
    k, it = ctypes.c_int64(), ctypes.c_int()
    _call(eng, "sl_segment_plane", _ptr(P) if n else None, n, float(distance_threshold), int(ransac_n),
          int(num_iterations), float(probability), int(seed) & ((1 << 64) - 1), int(batch),
          plane.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), inl.data_ptr(), ctypes.byref(k), rest.data_ptr(),
          ctypes.byref(it))
    return plane, inl[: k.value], {"iterations": it.value, "rest": rest[: n - k.value]}


# ---------------------------------------------------- density clustering ----
# Old/StatisticalOutlierRemoval.py's second recipe (remove_outliers_keep_color2):
# compute_nearest_neighbor_distance, keep_largest_cluster(cluster_dbscan) and
# remove_radius_outlier.  Open3D's algorithms restated (csrc/slcluster.inl);
# parity with Open3D is unpinned and tests/cluster_oracle.py is the restatement
# the tests check against, exactly.  A neighbour of i is a point with
# ((dx dx + dy dy) + dz dz) < r r (f64, in that order), i itself included.
def radius_count(points, radius: float, cap: int = 0, *, device=None) -> torch.Tensor:
    """min(neighbour count within ``radius``, ``cap``) of every point
    (sl_radius_count; ``cap <= 0``: the exact count) -> int32 [N] on the device."""
    eng = _engine(device)
    P = _f64(points, eng.device)
    n = P.shape[0]
    cnt = torch.empty(max(n, 1), dtype=torch.int32, device=eng.device)
    _call(eng, "sl_radius_count", _ptr(P) if n else None, n, float(radius), int(cap), cnt.data_ptr())
    return cnt[:n]


def cluster_dbscan(points, eps: float, min_points: int, *, device=None, info: bool = False):
    """PointCloud.cluster_dbscan(eps, min_points) (sl_cluster_dbscan) -> labels
    int32 [N] on the device: -1 noise, else the cluster, numbered by its
    smallest core index; a border point takes the smallest label among its core
    neighbours' clusters.  With ``info``: also {"clusters", "core", "noise"}
    (the core points are counted by one more capped radius_count)."""
    eng = _engine(device)
    P = _f64(points, eng.device)
    n = P.shape[0]
    labels = torch.empty(max(n, 1), dtype=torch.int32, device=eng.device)
    k = ctypes.c_int64()
    _call(eng, "sl_cluster_dbscan", _ptr(P) if n else None, n, float(eps), int(min_points), labels.data_ptr(),
          ctypes.byref(k))
    labels = labels[:n]
    if not info:
        return labels
    core = int((radius_count(P, eps, min_points, device=eng.device) >= int(min_points)).sum()) if n else 0
    return labels, {"clusters": k.value, "core": core, "noise": int((labels < 0).sum())}


def remove_radius_outlier(points, nb_points: int, radius: float, *, device=None) -> torch.Tensor:
    """PointCloud.remove_radius_outlier(nb_points, radius) -> the indices
    (int64, ascending, on the device) of the points with more than ``nb_points``
    neighbours within ``radius``, themselves included; pass them to
    ``select_by_index``."""
    if nb_points < 1 or not radius > 0:
        raise ValueError("Illegal input parameters, number of points and radius must be positive")
    cnt = radius_count(points, radius, int(nb_points) + 1, device=device)
    return torch.nonzero(cnt > int(nb_points)).reshape(-1)


def compute_nearest_neighbor_distance(points, *, device=None) -> torch.Tensor:
    """PointCloud.compute_nearest_neighbor_distance() (sl_nearest_neighbor_
    distance) -> f64 [N] on the device: the distance to the nearest other point
    (0 for a duplicated point and for a cloud of one point)."""
    eng = _engine(device)
    P = _f64(points, eng.device)
    n = P.shape[0]
    out = torch.empty(max(n, 1), dtype=torch.float64, device=eng.device)
    _call(eng, "sl_nearest_neighbor_distance", _ptr(P) if n else None, n, out.data_ptr())
    return out[:n]


def largest_cluster_label(labels) -> int | None:
    """The label >= 0 with the most points, the lowest on equal counts (np.unique
    sorts and ``counts.argmax()`` takes the first); None when there is none.
    The histogram and its first maximum are computed where ``labels`` lives."""
    L = torch.as_tensor(labels)
    L = L[L >= 0].to(torch.int64)
    if L.numel() == 0:
        return None
    counts = torch.bincount(L)
    return int(torch.nonzero(counts == counts.max()).reshape(-1)[0])  # the first index equal to the max


def keep_largest_cluster(points, colors=None, eps: float = 5, min_points: int = 200, *, device=None):
    """keep_largest_cluster (Old/StatisticalOutlierRemoval.py:5-32): the points
    of cluster_dbscan's most populous cluster -> (points, colors | None) on the
    device; an empty cloud, or one that is all noise, comes back unchanged."""
    eng = _engine(device)
    P = _f64(points, eng.device)
    C = _u8(colors, eng.device, P.shape[0])
    if P.shape[0] == 0:
        return P, C
    labels = cluster_dbscan(P, eps, min_points, device=eng.device)
    best = largest_cluster_label(labels)
    if best is None:
        return P, C
    return select_by_index(P, C, torch.nonzero(labels == best).reshape(-1), device=eng.device)


def cluster_dbscan_stage_ms(*, device=None) -> dict:
    """Host milliseconds per stage of this thread's last cluster_dbscan
    (sl_cluster_dbscan_stats; a measurement aid)."""
    eng = _engine(device)
    ms = (ctypes.c_double * 5)()
    _lib.check(eng._L.sl_cluster_dbscan_stats(ms, 5), None, "sl_cluster_dbscan_stats")
    return dict(zip(("grid", "count", "union", "rank", "border"), ms))


def transform(points, pose, *, device=None) -> torch.Tensor:
    """PointCloud.transform(pose) on a device copy of points (row order ((m0 x + m1 y) + m2 z) + m3)."""
    eng = _engine(device)
    P = _f64(points, eng.device).clone()
    M = torch.as_tensor(np.asarray(pose, dtype=np.float64).reshape(16)).to(eng.device)
    _call(eng, "sl_transform_points", P.data_ptr(), P.shape[0], M.data_ptr())
    return P


def estimate_normals(points, radius: float, max_nn: int = 30, *, device=None) -> torch.Tensor:
    """PointCloud.estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) of a
    cloud without normals (processing.py:178) -> normals f64 [N,3] on the
    device (sl_estimate_normals; max_nn <= 32)."""
    eng = _engine(device)
    P = _f64(points, eng.device)
    n = P.shape[0]
    out = torch.empty((max(n, 1), 3), dtype=torch.float64, device=eng.device)
    _call(eng, "sl_estimate_normals", _ptr(P), n, float(radius), int(max_nn), out.data_ptr())
    return out[:n]


def registration_icp(source, target, target_normals, max_correspondence_distance: float, init=None, *,
                     max_iteration: int = 30, relative_fitness: float = 1e-6, relative_rmse: float = 1e-6,
                     device=None) -> dict:
    """o3d.pipelines.registration.registration_icp(source, target,
    max_correspondence_distance, init, TransformationEstimationPointToPlane(),
    ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration))
    (processing.py:154-156) on the GPU -> {"transformation": 4x4 numpy,
    "fitness", "inlier_rmse", "iterations"}.  ``target_normals``: the target's
    normals (estimate_normals, as merge_pro_360 computes them)."""
    eng = _engine(device)
    S = _f64(source, eng.device)
    T = _f64(target, eng.device)
    N = _f64(target_normals, eng.device)
    if N.shape != T.shape:
        raise ValueError("TransformationEstimationPointToPlane requires pre-computed normal vectors for the "
                         "target point cloud")
    M0 = np.ascontiguousarray(np.eye(4) if init is None else np.asarray(init, dtype=np.float64).reshape(4, 4))
    out = np.zeros(16)
    fit, rmse, it = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
    _call(eng, "sl_icp_point_to_plane", _ptr(S) if len(S) else None, S.shape[0], _ptr(T) if len(T) else None,
          _ptr(N) if len(N) else None, T.shape[0], float(max_correspondence_distance), M0.ctypes.data,
          int(max_iteration), float(relative_fitness), float(relative_rmse), out.ctypes.data, ctypes.byref(fit),
          ctypes.byref(rmse), ctypes.byref(it))
    return {"transformation": out.reshape(4, 4), "fitness": fit.value, "inlier_rmse": rmse.value,
            "iterations": it.value}


def radius_search(points, radius: float, max_nn: int, *, device=None):
    """KDTreeFlann.search_hybrid_vector_3d of every point (sl_radius_search)
    -> (idx int32 [N, max_nn], d2 f64 [N, max_nn], count int32 [N]) on the
    device; row i's first count[i] entries, ascending (d2, index)."""
    eng = _engine(device)
    P = _f64(points, eng.device)
    n = P.shape[0]
    idx = torch.empty((max(n, 1), max_nn), dtype=torch.int32, device=eng.device)
    d2 = torch.empty((max(n, 1), max_nn), dtype=torch.float64, device=eng.device)
    cnt = torch.empty(max(n, 1), dtype=torch.int32, device=eng.device)
    _call(eng, "sl_radius_search", _ptr(P), n, float(radius), int(max_nn), idx.data_ptr(), d2.data_ptr(),
          cnt.data_ptr())
    return idx[:n], d2[:n], cnt[:n]


def compute_fpfh_feature(points, normals, radius: float, max_nn: int = 100, *, device=None) -> torch.Tensor:
    """o3d.pipelines.registration.compute_fpfh_feature(pcd,
    KDTreeSearchParamHybrid(radius, max_nn)) (processing.py:91-94) ->
    features f64 [N, 33] on the device (Open3D's Feature.data transposed)."""
    eng = _engine(device)
    P = _f64(points, eng.device)
    N = _f64(normals, eng.device)
    if N.shape != P.shape:
        raise ValueError("compute_fpfh_feature needs a normal per point")
    n = P.shape[0]
    out = torch.empty((max(n, 1), 33), dtype=torch.float64, device=eng.device)
    _call(eng, "sl_compute_fpfh", _ptr(P), _ptr(N), n, float(radius), int(max_nn), out.data_ptr())
    return out[:n]


def feature_nn(a, b, *, device=None) -> torch.Tensor:
    """Nearest row of ``b`` for every row of ``a`` (33-D features,
    sl_feature_nn) -> int32 [len(a)] on the device."""
    eng = _engine(device)
    A = torch.as_tensor(a).to(device=eng.device, dtype=torch.float64).contiguous()
    B = torch.as_tensor(b).to(device=eng.device, dtype=torch.float64).contiguous()
    if A.dim() != 2 or B.dim() != 2 or A.shape[1] != 33 or B.shape[1] != 33:
        raise ValueError("features must be [N, 33]")
    out = torch.empty(max(A.shape[0], 1), dtype=torch.int32, device=eng.device)
    _call(eng, "sl_feature_nn", _ptr(A), A.shape[0], _ptr(B), B.shape[0], 33, out.data_ptr())
    return out[:A.shape[0]]


def registration_ransac_based_on_feature_matching(source, target, source_feature, target_feature,
                                                  mutual_filter: bool, max_correspondence_distance: float, *,
                                                  edge_similarity: float = 0.9, max_iteration: int = 100000,
                                                  confidence: float = 0.999, seed: int = 0, device=None) -> dict:
    """o3d.pipelines.registration.registration_ransac_based_on_feature_matching
    (source, target, source_fpfh, target_fpfh, mutual_filter,
    max_correspondence_distance, TransformationEstimationPointToPoint(False),
    3, [CorrespondenceCheckerBasedOnEdgeLength(edge_similarity),
    CorrespondenceCheckerBasedOnDistance(max_correspondence_distance)],
    RANSACConvergenceCriteria(max_iteration, confidence)) (processing.py:
    98-111) on the GPU (sl_ransac_feature_matching; ``seed`` fixes the draw,
    which Open3D leaves unseeded) -> {"transformation": 4x4 numpy, "fitness",
    "inlier_rmse", "iterations", "validations", "correspondences"}."""
    eng = _engine(device)
    S = _f64(source, eng.device)
    T = _f64(target, eng.device)
    FS = torch.as_tensor(source_feature).to(device=eng.device, dtype=torch.float64).contiguous()
    FT = torch.as_tensor(target_feature).to(device=eng.device, dtype=torch.float64).contiguous()
    if FS.shape != (S.shape[0], 33) or FT.shape != (T.shape[0], 33):
        raise ValueError("features must be [N, 33], one row per point")
    out = np.zeros(16)
    fit, rmse = ctypes.c_double(), ctypes.c_double()
    it, vals, nc = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    _call(eng, "sl_ransac_feature_matching", _ptr(S) if len(S) else None, S.shape[0], _ptr(T) if len(T) else None,
          T.shape[0], _ptr(FS) if len(FS) else None, _ptr(FT) if len(FT) else None, int(bool(mutual_filter)),
          float(max_correspondence_distance), float(edge_similarity), int(max_iteration), float(confidence),
          int(seed) & ((1 << 64) - 1), out.ctypes.data, ctypes.byref(fit), ctypes.byref(rmse), ctypes.byref(it),
          ctypes.byref(vals), ctypes.byref(nc))
    return {"transformation": out.reshape(4, 4), "fitness": fit.value, "inlier_rmse": rmse.value,
            "iterations": it.value, "validations": vals.value, "correspondences": nc.value}


def preprocess_point_cloud(points, voxel_size: float, *, device=None):
    """preprocess_point_cloud (processing.py:79-96): voxel_down_sample, normals
    (radius 2 voxel, max_nn 30), FPFH (radius 5 voxel, max_nn 100) ->
    (down points, their normals, their features) on the device."""
    Pd, _ = voxel_down_sample(points, None, voxel_size, device=device)
    Nd = estimate_normals(Pd, voxel_size * 2, 30, device=device)
    Fd = compute_fpfh_feature(Pd, Nd, voxel_size * 5, 100, device=device)
    return Pd, Nd, Fd


def execute_global_registration(source_down, target_down, source_fpfh, target_fpfh, voxel_size: float, *,
                                seed: int = 0, device=None) -> dict:
    """execute_global_registration (processing.py:98-113): RANSAC on FPFH
    matches with the reference's settings (mutual filter, distance 1.5 voxel,
    edge length 0.9, 100000 iterations, confidence 0.999)."""
    return registration_ransac_based_on_feature_matching(
        source_down, target_down, source_fpfh, target_fpfh, True, voxel_size * 1.5, edge_similarity=0.9,
        max_iteration=100000, confidence=0.999, seed=seed, device=device)


def rigid_inverse(M) -> np.ndarray:
    """[R | t]^-1 = [R^T | -(R^T t)] of a rigid 4x4 pose."""
    M = np.asarray(M, dtype=np.float64).reshape(4, 4)
    R, t = M[:3, :3], M[:3, 3]
    out = np.zeros((4, 4))
    out[:3, :3] = R.T
    for i in range(3):
        out[i, 3] = -((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2])
    out[3, 3] = 1.0
    return out


def mat4(a, b) -> np.ndarray:
    """Row-major 4x4 product ((a0 b0 + a1 b1) + a2 b2) + a3 b3 (np.dot of
    processing.py:162, in a fixed order)."""
    a = np.asarray(a, dtype=np.float64).reshape(4, 4)
    b = np.asarray(b, dtype=np.float64).reshape(4, 4)
    out = np.empty((4, 4))
    for i in range(4):
        for j in range(4):
            out[i, j] = ((a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j]) + a[i, 3] * b[3, j]
    return out


def merge_pro_360(input_folder, output_path, voxel_size: float = 0.02, *, seed_poses=None, device=None,
                  binary: bool = True, order: str = "lexicographic", max_iteration: int = 30,
                  return_transforms: bool = False, ransac_seed: int = 0):
    """merge_pro_360 (processing.py:116-182): the clouds of ``input_folder``
    (``ply_files(order)``; default the reference's lexicographic order)
    registered in sequence -- scan i onto scan i-1 by point-to-plane ICP
    between their voxel-downsampled clouds (target normals radius 2 voxel,
    max_nn 30; max correspondence distance = voxel_size; :145-157), the
    transforms accumulated T_i = T_{i-1} T_local (:159-167) and scan i moved
    by T_i -- then merged, voxel-downsampled, outlier-filtered, normals
    estimated and written in Open3D's layout (as merge_pro_360_posed).

    Each ICP starts, as the reference's, from the FPFH + RANSAC global
    estimate (preprocess_point_cloud / execute_global_registration, :79-113:
    FPFH radius 5 voxel, RANSAC distance 1.5 voxel; ``ransac_seed`` fixes its
    draw), unless ``seed_poses`` is given: then from ``inverse(seed_poses[i-1])
    @ seed_poses[i]`` (the turntable's relative pose between the two views;
    poses mapping each view into a common frame, e.g. synth.turntable_pose).
    Returns (points, colors, normals) on the device (+ the accumulated
    transforms with ``return_transforms``)."""
    print(f"[Merge 360] Loading clouds from {input_folder}...")
    files = ply_files(input_folder, order)
    if len(files) < 2:
        raise ValueError("Need at least 2 .ply files to merge.")
    if seed_poses is not None:
        seed_poses = np.asarray(seed_poses, dtype=np.float64).reshape(-1, 4, 4)
        if len(seed_poses) != len(files):
            raise ValueError(f"{len(files)} clouds but {len(seed_poses)} seed poses")
    eng = _engine(device)
    pcds = []
    for f in files:
        pcds.append(_read_cloud(f, eng.device))
    print(f"[Merge 360] Loaded {len(pcds)} clouds. Running Sequential Registration (New360 Logic)...")
    down = {}

    def prep(i):  # preprocess_point_cloud (:79-96); the FPFH features only for RANSAC
        if i not in down:
            if seed_poses is None:
                down[i] = preprocess_point_cloud(pcds[i][0], voxel_size, device=eng.device)
            else:
                Pd, _ = voxel_down_sample(pcds[i][0], None, voxel_size, device=eng.device)
                down[i] = (Pd, estimate_normals(Pd, voxel_size * 2, 30, device=eng.device), None)
        return down[i]
    accum = np.eye(4)
    transforms = [accum.copy()]
    parts_p, parts_c = [pcds[0][0]], [pcds[0][1]]
    for i in range(1, len(pcds)):
        print(f"[Merge 360] Aligning Scan {i} -> Scan {i-1}...")
        src, _, src_f = prep(i)
        tgt, tgt_n, tgt_f = prep(i - 1)
        if seed_poses is None:  # execute_global_registration (:146-151)
            init = execute_global_registration(src, tgt, src_f, tgt_f, voxel_size, seed=ransac_seed + i,
                                               device=eng.device)["transformation"]
        else:
            init = mat4(rigid_inverse(seed_poses[i - 1]), seed_poses[i])
        T_local = registration_icp(src, tgt, tgt_n, voxel_size, init, max_iteration=max_iteration,
                                   device=eng.device)["transformation"]
        accum = mat4(accum, T_local)
        transforms.append(accum.copy())
        parts_p.append(transform(pcds[i][0], accum, device=eng.device))
        parts_c.append(pcds[i][1])
        down.pop(i - 1, None)
    P, C, N = _finish_merge(parts_p, parts_c, voxel_size, output_path, binary, eng.device)
    return (P, C, N, transforms) if return_transforms else (P, C, N)


def _finish_merge(parts_p, parts_c, voxel_size, output_path, binary, device):
    """processing.py:169-181: the moved clouds concatenated, post-processed, normals estimated (radius 2 voxel,
    max_nn 30) and written -> (points, colors, normals) on the device."""
    print("[Merge 360] Post-processing (Downsample + Outlier removal)...")
    P, C = postprocess(torch.cat(parts_p), torch.cat(parts_c), voxel_size, device=device)
    N = estimate_normals(P, voxel_size * 2, 30, device=device)
    ply.save_ply_open3d(P.cpu().numpy(), C.cpu().numpy(), output_path, normals=N.cpu().numpy(), binary=binary)
    print(f"[Merge 360] Saved merged cloud to {output_path}")
    return P, C, N


def pool_trim(device=None) -> int:
    """Release the merge kernels' pooled scratch buffers of ``device``
    (sl_merge_pool_trim); returns the bytes released."""
    eng = _engine(device)
    out = ctypes.c_int64()
    _lib.check(eng._L.sl_merge_pool_trim(eng.device.index, ctypes.byref(out)), None, "sl_merge_pool_trim")
    return out.value


_poison_lock = threading.Lock()
_poison_mode = -1  # the mode this module last set: -1 disarmed, else the byte


def _pool_poison_set(byte: int) -> int:
    """sl_merge_pool_poison(byte) -> the counter; the mode set is remembered.  Under _poison_lock."""
    global _poison_mode
    out = ctypes.c_int64()
    _lib.check(_lib.load().sl_merge_pool_poison(byte, ctypes.byref(out)), None,
               "sl_merge_pool_poison: byte must be 0..255, or -1 to disarm")
    _poison_mode = byte
    return out.value


class pool_poison:
    """Test aid (sl_merge_pool_poison): ``with merge.pool_poison(0xFF) as p:`` fills every scratch buffer
    the merge pool hands out inside the block with that byte before its entry point's first kernel; when
    the block ends the mode is what it was before it (disarmed, or an outer block's byte).  ``p.bytes()``
    is the process-wide count of bytes filled so far (never reset: use differences); reading it, inside or
    outside a block, leaves the mode alone (the C call reports the counter only while setting a mode, so
    the mode this module set last is set again: a mode set past this module, through ctypes, is not
    known here).  The mode is process-wide: blocks in several threads at once are not supported.
    Results must not depend on any of it."""

    def __init__(self, byte: int):
        self.byte = int(byte)
        self._before = -1

    def bytes(self) -> int:
        with _poison_lock:
            return _pool_poison_set(_poison_mode)

    def __enter__(self):
        with _poison_lock:
            before = _poison_mode
            _pool_poison_set(self.byte)  # ValueError for a byte outside 0..255: nothing changes
            self._before = before
        return self

    def __exit__(self, *exc):
        with _poison_lock:
            _pool_poison_set(self._before)
        return False


def postprocess(points, colors, voxel_size: float, nb_neighbors: int = 20, std_ratio: float = 2.0, *,
                device=None):
    """processing.py:171-175: voxel_down_sample, then remove_statistical_outlier + select_by_index."""
    P, C = voxel_down_sample(points, colors, voxel_size, device=device)
    ind, _ = remove_statistical_outlier(P, nb_neighbors, std_ratio, device=device)
    return select_by_index(P, C, ind, device=device)


def ply_files(folder, order: str = "lexicographic") -> list:
    """The clouds a 360 merge reads, in its order: ``"lexicographic"`` is
    processing.py:121's ``sorted(glob('*.ply'))`` (``view_100deg`` before
    ``view_10deg``); ``"numeric"`` is Old/new360Merge.py:7-20's key, the first
    integer in the file name (0 when none; ties keep name order)."""
    if order == "lexicographic":
        return sorted(glob.glob(os.path.join(folder, "*.ply")))
    if order == "numeric":
        names = sorted(f for f in os.listdir(folder) if f.lower().endswith(".ply"))

        def first_int(name):
            m = re.search(r"\d+", name)
            return int(m.group()) if m else 0
        return [os.path.join(folder, f) for f in sorted(names, key=first_int)]
    raise ValueError("order must be 'lexicographic' or 'numeric'")


def merge_pro_360_posed(input_folder, output_path, poses, voxel_size: float = 0.02, *, device=None,
                        binary: bool = True, order: str = "lexicographic"):
    """merge_pro_360 (processing.py:116-182) with known per-file poses instead
    of the FPFH/RANSAC/ICP estimate: files in ``ply_files(order)`` order
    (default: the reference's lexicographic one), file i moved by ``poses[i]``
    (4x4), merged, post-processed, normals estimated (radius 2 voxel, max_nn 30,
    :178) and written as o3d.io.write_point_cloud writes it (binary, double
    xyz + normals, uchar RGB: ply.save_ply_open3d; ``binary=False``: the same
    properties in ASCII).  Returns (points, colors, normals) on the device."""
    print(f"[Merge 360] Loading clouds from {input_folder}...")
    files = ply_files(input_folder, order)
    if len(files) < 2:
        raise ValueError("Need at least 2 .ply files to merge.")
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    if len(poses) != len(files):
        raise ValueError(f"{len(files)} clouds but {len(poses)} poses")
    eng = _engine(device)
    parts_p, parts_c = [], []
    for f, M in zip(files, poses):
        P, C = _read_cloud(f, eng.device)
        parts_p.append(transform(P, M, device=eng.device))
        parts_c.append(C)
    print(f"[Merge 360] Loaded {len(files)} clouds. Applying the given poses...")
    return _finish_merge(parts_p, parts_c, voxel_size, output_path, binary, eng.device)


# ------------------------------------------------- loop-closing 360 merge ----
# Old/new360Merge.py:77-178 (and Old/360Merge.py:19-84): every pair of
# neighbouring views and the closing pair (first, last) registered, each edge
# weighted by its information matrix, and the closing error spread over the
# ring by pose-graph optimisation.  Open3D's algorithms restated
# (csrc/slinfo.inl, csrc/slposegraph.inl); parity with Open3D is unpinned and
# tests/posegraph_oracle.py is the restatement the tests check against.
def get_information_matrix_from_point_clouds(source, target, max_correspondence_distance, transformation, *,
                                             info: bool = False, device=None):
    """o3d.pipelines.registration.get_information_matrix_from_point_clouds
    (source, target, max_correspondence_distance, transformation) on the GPU
    (sl_information_matrix) -> the 6x6 numpy matrix (with ``info``: also the
    number of correspondences)."""
    eng = _engine(device)
    S = _f64(source, eng.device)
    T = _f64(target, eng.device)
    M = np.ascontiguousarray(np.asarray(transformation, dtype=np.float64).reshape(4, 4))
    out = np.zeros((6, 6))
    cnt = ctypes.c_int64()
    _call(eng, "sl_information_matrix", _ptr(S) if len(S) else None, S.shape[0], _ptr(T) if len(T) else None,
          T.shape[0], float(max_correspondence_distance), M.ctypes.data, out.ctypes.data, ctypes.byref(cnt))
    return (out, cnt.value) if info else out


class PoseGraph:
    """o3d.pipelines.registration.PoseGraph: ``nodes``, a list of 4x4 poses
    (node frame -> the frame of node 0), and ``edges``, a list of (source_id,
    target_id, transformation 4x4 (source -> target), information 6x6,
    uncertain)."""

    def __init__(self, nodes=None, edges=None):
        self.nodes = [] if nodes is None else list(nodes)
        self.edges = [] if edges is None else list(edges)


# GlobalOptimizationConvergenceCriteria's defaults
POSE_GRAPH_CRITERIA = dict(max_iteration=100, min_relative_increment=1e-6, min_relative_residual_increment=1e-6,
                           min_right_term=1e-6, min_residual=1e-6, max_iteration_lm=20)


def global_optimization(pose_graph: PoseGraph, *, max_correspondence_distance, edge_prune_threshold: float = 0.25,
                        reference_node: int = 0, criteria=None) -> dict:
    """o3d.pipelines.registration.global_optimization(pose_graph,
    GlobalOptimizationLevenbergMarquardt(), criteria, GlobalOptimizationOption(
    max_correspondence_distance, edge_prune_threshold, reference_node))
    (Old/new360Merge.py:121-131) by sl_pose_graph_optimize: host code of the
    library, no GPU.  Updates ``pose_graph.nodes`` in place -> {"iterations",
    "initial_residual", "final_residual"} (the sum of e^T Lambda e over the
    edges).  ``criteria``: a dict overriding POSE_GRAPH_CRITERIA.

    Every edge must be certain, as the reference marks them: the line process
    and edge pruning are not implemented and an ``uncertain`` edge raises
    ValueError.  ``max_correspondence_distance`` and ``edge_prune_threshold``
    only steer those two in Open3D; they are accepted and unused."""
    unknown = set(criteria or {}) - set(POSE_GRAPH_CRITERIA)
    if unknown:
        raise ValueError(f"unknown criteria: {sorted(unknown)}")
    c = dict(POSE_GRAPH_CRITERIA, **(criteria or {}))
    n, m = len(pose_graph.nodes), len(pose_graph.edges)
    if any(e[4] for e in pose_graph.edges):
        raise ValueError("global_optimization: an edge is marked uncertain; the line process and edge pruning are "
                         "not implemented (every edge must be certain)")
    poses = np.ascontiguousarray(np.asarray(pose_graph.nodes, dtype=np.float64).reshape(n, 16))
    src = np.ascontiguousarray([e[0] for e in pose_graph.edges], dtype=np.int32)
    tgt = np.ascontiguousarray([e[1] for e in pose_graph.edges], dtype=np.int32)
    X = np.ascontiguousarray(np.asarray([e[2] for e in pose_graph.edges], dtype=np.float64).reshape(m, 16))
    L = np.ascontiguousarray(np.asarray([e[3] for e in pose_graph.edges], dtype=np.float64).reshape(m, 36))
    it, r0, r1 = ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
    code = _lib.load().sl_pose_graph_optimize(
        poses.ctypes.data, n, src.ctypes.data, tgt.ctypes.data, X.ctypes.data, L.ctypes.data, None, m,
        int(reference_node), int(c["max_iteration"]), int(c["max_iteration_lm"]), float(c["min_right_term"]),
        float(c["min_relative_increment"]), float(c["min_relative_residual_increment"]), float(c["min_residual"]),
        ctypes.byref(it), ctypes.byref(r0), ctypes.byref(r1))
    _lib.check(code, None, f"sl_pose_graph_optimize: {n} nodes, reference node {reference_node}: no node, a "
                           "reference node or an edge id out of range, or bad criteria")
    pose_graph.nodes[:] = [poses[i].reshape(4, 4).copy() for i in range(n)]
    return {"iterations": it.value, "initial_residual": r0.value, "final_residual": r1.value}


def full_registration(views, voxel_size: float, *, seed_poses=None, ransac_seed: int = 0, max_iteration: int = 30,
                      device=None) -> PoseGraph:
    """load_point_clouds' features and full_registration's loop
    (Old/new360Merge.py:37-62, 96-119) over ``views`` (clouds, [N, 3] each) ->
    the PoseGraph before optimisation.  Per view: normals of the full cloud
    (radius 2 voxel, max_nn 30), then preprocess_point_cloud.  For every pair
    (i, i + 1), and (0, n - 1) when n > 2, in the reference's order and with
    the lower id as the source: the global RANSAC estimate on the down-sampled
    clouds (``ransac_seed`` + the edge's number fixes its draw), point-to-plane
    ICP on the FULL clouds at 0.4 voxel from it, and the information matrix at
    0.4 voxel with the ICP's result; node k + 1 is the inverse of the
    accumulated odometry.  With ``seed_poses`` (poses mapping each view into a
    common frame, as merge_pro_360 takes them) the RANSAC estimate is replaced
    by ``inverse(seed_poses[t]) @ seed_poses[s]`` and the down-sampled clouds
    and features, which only RANSAC reads, are not computed."""
    eng = _engine(device)
    clouds = [_f64(v, eng.device) for v in views]
    n = len(clouds)
    if seed_poses is not None:
        seed_poses = np.asarray(seed_poses, dtype=np.float64).reshape(-1, 4, 4)
        if len(seed_poses) != n:
            raise ValueError(f"{n} clouds but {len(seed_poses)} seed poses")
    print(f"Found {n} scans. Extracting geometric features...")
    normals = [estimate_normals(P, voxel_size * 2, 30, device=eng.device) for P in clouds]
    down = [preprocess_point_cloud(P, voxel_size, device=eng.device) for P in clouds] if seed_poses is None else None
    graph = PoseGraph([np.eye(4)])
    odometry = np.eye(4)
    distance = voxel_size * 0.4
    for s in range(n):
        for t in range(s + 1, n):
            if not (t == s + 1 or (s == 0 and t == n - 1)):
                continue
            print(f"\nAligning scan {s} to {t}...")
            if seed_poses is None:
                print("  -> Running Global Registration (RANSAC)...")
                init = execute_global_registration(down[s][0], down[t][0], down[s][2], down[t][2], voxel_size,
                                                   seed=ransac_seed + len(graph.edges),
                                                   device=eng.device)["transformation"]
            else:
                init = mat4(rigid_inverse(seed_poses[t]), seed_poses[s])
            print("  -> Running Fine ICP...")
            T_icp = registration_icp(clouds[s], clouds[t], normals[t], distance, init, max_iteration=max_iteration,
                                     device=eng.device)["transformation"]
            information = get_information_matrix_from_point_clouds(clouds[s], clouds[t], distance, T_icp,
                                                                   device=eng.device)
            if t == s + 1:
                odometry = mat4(T_icp, odometry)
                graph.nodes.append(rigid_inverse(odometry))
            graph.edges.append((s, t, T_icp, information, False))
    return graph


def merge_360_pose_graph(input_folder, output_path, voxel_size: float = 1.0, *, order: str = "numeric",
                         seed_poses=None, ransac_seed: int = 0, binary: bool = True, return_graph: bool = False,
                         device=None):
    """Old/new360Merge.py:152-178, the loop-closing 360 merge: the clouds of
    ``input_folder`` (``ply_files(order)``; default the script's numeric order)
    through ``full_registration``, then ``global_optimization`` (0.4 voxel,
    0.25, reference node 0), every view moved by its node's pose, the views
    concatenated, down-sampled at 0.5 voxel, filtered by
    remove_statistical_outlier(20, 2.0), normals estimated, and written in
    Open3D's layout (ply.save_ply_open3d).  The script's bare
    ``estimate_normals()`` is Open3D's default, a 30-nearest-neighbour search;
    here the normals are merge_pro_360's (radius 2 voxel, max_nn 30).  Returns
    (points, colors, normals) on the device (+ the optimised PoseGraph with
    ``return_graph``).  The Poisson mesh the script appends is ``mesh_360`` on
    the written file."""
    files = ply_files(input_folder, order)
    if len(files) < 2:
        raise ValueError("Need at least 2 .ply files to merge.")
    eng = _engine(device)
    pcds = []
    for f in files:
        pcds.append(_read_cloud(f, eng.device))
    graph = full_registration([p for p, _ in pcds], voxel_size, seed_poses=seed_poses, ransac_seed=ransac_seed,
                              device=eng.device)
    print("\nRunning Pose Graph Optimization...")
    global_optimization(graph, max_correspondence_distance=voxel_size * 0.4, edge_prune_threshold=0.25,
                        reference_node=0)
    print("Transforming points...")
    parts_p = [transform(p, graph.nodes[i], device=eng.device) for i, (p, _) in enumerate(pcds)]
    print("\nMerging point clouds...")
    print("Post-processing (Removing noise)...")
    P, C = postprocess(torch.cat(parts_p), torch.cat([c for _, c in pcds]), voxel_size * 0.5, 20, 2.0,
                       device=eng.device)
    N = estimate_normals(P, voxel_size * 2, 30, device=eng.device)
    print("Saving merged point cloud...")
    ply.save_ply_open3d(P.cpu().numpy(), C.cpu().numpy(), output_path, normals=N.cpu().numpy(), binary=binary)
    print(f"Point cloud saved to {output_path}")
    return (P, C, N, graph) if return_graph else (P, C, N)
