"""Drop-in for the reference's ``Old/StatisticalOutlierRemoval.py``.

    python -m structured_light_for_3d_model_replication_amd.statistical_outlier_removal IN.ply OUT.ply

The two per-view cleaning recipes of that script, with its names, arguments,
defaults and prints, on the GPU through ``merge`` (libslgpu.so):

* ``remove_outliers_keep_color1`` (:34-72): ``remove_statistical_outlier`` +
  ``select_by_index``.
* ``remove_outliers_keep_color2`` (:74-116), the one its ``__main__`` runs:
  ``compute_nearest_neighbor_distance`` (its mean is printed),
  ``keep_largest_cluster`` (``cluster_dbscan(eps=5, min_points=200)``, then the
  most populous cluster) and ``remove_radius_outlier(nb_points=5, radius=15)``.
  As in the reference, ``nb_neighbors`` and ``std_ratio`` are accepted and
  unused by this recipe.
* ``keep_largest_cluster`` (:5-32) takes and returns a ``processing.Cloud``.

The clustering, the radius filter and the distances are csrc/slcluster.inl;
Open3D's algorithms restated, parity with Open3D unpinned (not in this image),
tests/cluster_oracle.py the CPU restatement.

Without Open3D a point cloud is a ``processing.Cloud`` of device tensors; files
are read with ``ply.read_cloud_device`` and written with ``ply.save_ply_open3d`` (the
layout o3d.io.write_point_cloud writes), colours kept.  Left out: the
``draw_geometries`` preview that ends both recipes (a GUI window) with its
"Visualizing..." line, and ``cluster_dbscan``'s progress bar.  A file without
colour prints the reference's warning and is written with black colours
(Open3D writes no colour properties).
"""
from __future__ import annotations

import argparse

import numpy as np

from . import merge, ply
from .processing import Cloud, _write


def _read(file_path) -> Cloud:
    """o3d.io.read_point_cloud: a ``Cloud`` on the device, ``colors`` None when the file has none."""
    cloud = ply.read_cloud_device(file_path, device=merge._engine(None).device)  # one read: colours or None
    return Cloud(cloud["points"], cloud["colors"])


def keep_largest_cluster(pcd: Cloud, eps=5, min_points=200) -> Cloud:
    print("Clustering points...")
    return Cloud(*merge.keep_largest_cluster(pcd.points, pcd.colors, eps=eps, min_points=min_points,
                                             device=pcd.points.device))


def _select_and_save(pcd: Cloud, ind, out) -> Cloud:
    """Steps 2 and 3 of both recipes: the inliers selected, the counts printed, the cloud written."""
    inlier_cloud = Cloud(*merge.select_by_index(pcd.points, pcd.colors, ind, device=pcd.points.device))
    print(f"Cleaned points: {len(inlier_cloud.points)}")
    print(f"Removed points: {len(pcd.points) - len(inlier_cloud.points)}")
    _write(out, inlier_cloud)
    print(f"Saved cleaned cloud with colors to: {out}")
    return inlier_cloud


def remove_outliers_keep_color1(file_path, out, nb_neighbors=20, std_ratio=2.0):
    print(f"Loading {file_path}...")
    pcd = _read(file_path)
    if pcd.colors is None:
        print("Warning: The input file does not have color data.")
    print("Removing outliers...")
    ind, _ = merge.remove_statistical_outlier(pcd.points, nb_neighbors=nb_neighbors, std_ratio=std_ratio,
                                              device=pcd.points.device)
    _select_and_save(pcd, ind, out)


def remove_outliers_keep_color2(file_path, out, nb_neighbors=20, std_ratio=2.0):
    print(f"Loading {file_path}...")
    pcd = _read(file_path)
    distances = merge.compute_nearest_neighbor_distance(pcd.points, device=pcd.points.device)
    avg_dist = np.mean(distances.cpu().numpy())
    print(f"Average point distance: {avg_dist}")
    pcd = keep_largest_cluster(pcd)
    if pcd.colors is None:
        print("Warning: The input file does not have color data.")
    print("Removing outliers...")
    ind = merge.remove_radius_outlier(pcd.points, nb_points=5, radius=15, device=pcd.points.device)
    _select_and_save(pcd, ind, out)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="Clean one view: largest DBSCAN cluster + radius outlier removal "
                                             "(recipe 2, the reference's default) or statistical outlier removal "
                                             "(recipe 1)")
    ap.add_argument("input", help="input .ply")
    ap.add_argument("output", help="output .ply")
    ap.add_argument("--recipe", type=int, choices=(1, 2), default=2)
    ap.add_argument("--nb-neighbors", type=int, default=20)
    ap.add_argument("--std-ratio", type=float, default=2.0)
    a = ap.parse_args(argv)
    run = remove_outliers_keep_color1 if a.recipe == 1 else remove_outliers_keep_color2
    run(a.input, a.output, nb_neighbors=a.nb_neighbors, std_ratio=a.std_ratio)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
