"""Density clustering on the GPU (csrc/slcluster.inl): sl_radius_count,
sl_cluster_dbscan and sl_nearest_neighbor_distance against tests/cluster_oracle.py,
exactly, and the ``statistical_outlier_removal`` drop-in built on them.  Open3D
is not installed: parity with Open3D is unpinned; the oracle's order-free DBSCAN
is shown equal to ClusterDBSCAN's sequential loop in tests/test_cluster_oracle.py.
Every result is computed twice and must repeat (the union-find is lock-free:
the interleaving differs from run to run, the labels may not)."""
import numpy as np
import pytest
import torch

from oracle import merge_oracle
from tests import cluster_oracle as co

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mg():
    from structured_light_for_3d_model_replication_amd import merge
    return merge


def _twice(fn):
    a, b = fn(), fn()
    a = a.cpu().numpy()
    np.testing.assert_array_equal(a, b.cpu().numpy())
    return a


@pytest.mark.parametrize("name", sorted(co.CASES))
def test_dbscan_matches_the_oracle(mg, name):
    s = co.solved(name)
    got = []
    for _ in range(2):
        labels, info = mg.cluster_dbscan(s["P"], s["eps"], s["min_points"], info=True)
        assert labels.dtype == torch.int32 and labels.is_cuda
        assert info == s["info"]
        got.append(labels.cpu().numpy())
    np.testing.assert_array_equal(got[0], got[1])
    np.testing.assert_array_equal(got[0], s["labels"])


@pytest.mark.parametrize("name", sorted(co.CASES))
def test_radius_count_matches_the_oracle(mg, name):
    s = co.solved(name)
    cnt = _twice(lambda: mg.radius_count(s["P"], s["eps"]))
    assert cnt.dtype == np.int32
    np.testing.assert_array_equal(cnt, s["counts"])


@pytest.mark.parametrize("cap", [1, 64, 200, 0])
def test_radius_count_cap_sweep_on_the_dense_cell(mg, cap):
    s = co.solved("dense_cell")
    assert s["counts"].max() >= 3000  # more than an LDS tile, many times over
    want = np.minimum(s["counts"], cap) if cap > 0 else s["counts"]
    np.testing.assert_array_equal(_twice(lambda: mg.radius_count(s["P"], s["eps"], cap)), want)


def test_trivial_sizes(mg):
    assert mg.cluster_dbscan(np.zeros((0, 3)), 1.0, 5).shape == (0,)
    assert mg.radius_count(np.zeros((0, 3)), 1.0).shape == (0,)
    assert mg.compute_nearest_neighbor_distance(np.zeros((0, 3))).shape == (0,)
    labels, info = mg.cluster_dbscan(np.array([[1.0, 2.0, 3.0]]), 1.0, 1, info=True)
    assert labels.tolist() == [0] and info == {"clusters": 1, "core": 1, "noise": 0}
    labels, info = mg.cluster_dbscan(np.array([[1.0, 2.0, 3.0]]), 1.0, 2, info=True)
    assert labels.tolist() == [-1] and info == {"clusters": 0, "core": 0, "noise": 1}
    s = co.solved("fewer_than_min_points")
    assert (mg.cluster_dbscan(s["P"], s["eps"], s["min_points"]) == -1).all()
    s = co.solved("min_points_one")
    labels = mg.cluster_dbscan(s["P"], s["eps"], 1)
    assert int(labels.min()) == 0 and int(labels.max()) + 1 == s["info"]["clusters"]
    s = co.solved("one_ball")
    assert (mg.radius_count(s["P"], s["eps"]) == 5000).all()
    assert (mg.cluster_dbscan(s["P"], s["eps"], s["min_points"]) == 0).all()
    assert (mg.radius_count(co.solved("identical")["P"], 0.5) == 300).all()


def test_strict_boundary(mg):
    P = co.lattice()
    closed, opened = 1.0, float(np.nextafter(1.0, 2.0))
    assert (mg.radius_count(P, closed) == 1).all()  # points exactly 1 apart are not neighbours
    inner = ((P > 0) & (P < [5, 4, 3])).all(1)
    cnt = mg.radius_count(P, opened).cpu().numpy()
    assert (cnt[inner] == 7).all() and cnt.min() == 4
    assert (mg.cluster_dbscan(P, closed, 2) == -1).all()
    assert (mg.cluster_dbscan(P, opened, 2) == 0).all()


@pytest.mark.parametrize("order", ["a", "b"])
def test_contested_border(mg, order):
    P, eps, mp, bridge = co.bridge_rows(order)
    cnt = mg.radius_count(P, eps).cpu().numpy()
    labels = _twice(lambda: mg.cluster_dbscan(P, eps, mp))
    assert cnt[bridge] == 3 < mp  # not core
    d2 = ((P - P[bridge]) ** 2).sum(1)
    core_nb = np.nonzero((d2 < eps * eps) & (cnt >= mp))[0]
    assert sorted(labels[core_nb]) == [0, 1]  # core neighbours in two clusters
    assert labels[bridge] == 0                # the lower label
    np.testing.assert_array_equal(labels, co.dbscan_sequential(P, eps, mp))


def test_blobs_and_noise_has_every_kind(mg):
    s = co.solved("blobs_and_noise")
    labels, info = mg.cluster_dbscan(s["P"], s["eps"], s["min_points"], info=True)
    assert info == s["info"] and all(v > 0 for v in info.values())
    assert int((labels >= 0).sum()) > info["core"]  # border points


@pytest.mark.parametrize("name,nb_points", [("dense_cell", 5), ("blobs_and_noise", 9), ("duplicates", 1),
                                            ("wide_extent", 20), ("identical", 299), ("identical", 300),
                                            ("lattice_closed", 1), ("lattice_open", 4), ("single", 1)])
def test_remove_radius_outlier(mg, name, nb_points):
    s = co.solved(name)
    ind = _twice(lambda: mg.remove_radius_outlier(s["P"], nb_points, s["eps"]))
    assert ind.dtype == np.int64
    np.testing.assert_array_equal(ind, co.remove_radius_outlier(s["P"], nb_points, s["eps"], A=s["A"]))


@pytest.mark.parametrize("name", ["single", "identical", "duplicates", "lattice_open", "wide_extent", "dense_cell",
                                  "blobs_and_noise", "bridge_a"])
def test_nearest_neighbor_distance(mg, name):
    P = co.solved(name)["P"]
    d = _twice(lambda: mg.compute_nearest_neighbor_distance(P))
    want = co.nearest_neighbor_distance(P)
    np.testing.assert_array_equal(d, want)
    if name in ("identical", "single"):
        assert (d == 0).all()
    if name == "duplicates":
        assert (d[:50] == 0).all() and (d[-50:] == 0).all() and (d[50:-50] > 0).all()


@pytest.mark.parametrize("name", ["dense_cell", "equal_twins", "blobs_and_noise", "fewer_than_min_points"])
def test_keep_largest_cluster(mg, name):
    s = co.solved(name)
    P = s["P"]
    C = np.random.default_rng(0).integers(0, 256, (len(P), 3), dtype=np.uint8)
    keep = co.keep_largest_cluster(s["labels"])
    if name == "equal_twins":  # equal counts: the lowest label
        np.testing.assert_array_equal(keep, np.nonzero(s["labels"] == 0)[0])
    if name == "fewer_than_min_points":  # all noise: unchanged
        assert len(keep) == len(P)
    if name == "dense_cell":  # the largest cluster is not the first
        assert s["labels"][keep[0]] > 0
    for _ in range(2):
        Q, Cq = mg.keep_largest_cluster(P, C, s["eps"], s["min_points"])
        np.testing.assert_array_equal(Q.cpu().numpy(), P[keep])
        np.testing.assert_array_equal(Cq.cpu().numpy(), C[keep])
    Q, Cq = mg.keep_largest_cluster(np.zeros((0, 3)), None)
    assert Q.shape == (0, 3) and Cq is None
    assert mg.largest_cluster_label(torch.tensor([1, 0, 0, 1, -1])) == 0
    assert mg.largest_cluster_label(torch.tensor([-1, -1])) is None


def test_error_messages(mg):
    P = np.random.default_rng(0).uniform(0, 1, (10, 3))
    with pytest.raises(ValueError, match=r"^Illegal input parameters, number of points and radius must be positive$"):
        mg.remove_radius_outlier(P, 0, 1.0)
    with pytest.raises(ValueError, match=r"^Illegal input parameters, number of points and radius must be positive$"):
        mg.remove_radius_outlier(P, 5, 0.0)
    with pytest.raises(ValueError, match="eps must be positive"):
        mg.cluster_dbscan(P, 0.0, 5)
    with pytest.raises(ValueError, match="eps must be positive"):
        mg.cluster_dbscan(P, float("nan"), 5)
    with pytest.raises(ValueError, match="min_points must be at least 1"):
        mg.cluster_dbscan(P, 1.0, 0)
    with pytest.raises(ValueError, match="radius must be positive"):
        mg.radius_count(P, -1.0)
    for bad in (np.nan, np.inf):
        Q = P.copy()
        Q[3, 1] = bad
        with pytest.raises(ValueError, match="non-finite point coordinates"):
            mg.cluster_dbscan(Q, 1.0, 5)
        with pytest.raises(ValueError, match="non-finite point coordinates"):
            mg.radius_count(Q, 1.0)
        with pytest.raises(ValueError, match="non-finite point coordinates"):
            mg.compute_nearest_neighbor_distance(Q)
    # the engine still works after the errors
    assert (mg.radius_count(P, 10.0) == 10).all()


# ---- the drop-in for Old/StatisticalOutlierRemoval.py ----
def _view():
    """An object, a detached clump (locally dense: a statistical filter keeps it) and stray points, at
    the scale of the reference's parameters (eps 5, min_points 200, radius 15)."""
    rng = np.random.default_rng(11)
    P = np.concatenate([rng.normal(size=(1500, 3)) * 3.0, rng.normal(size=(400, 3)) * 1.5 + [60.0, 0.0, 0.0],
                        rng.uniform(-100, 100, (100, 3))])
    P = P[rng.permutation(len(P))]
    return P, rng.integers(0, 256, (len(P), 3), dtype=np.uint8)


def test_drop_in_recipe_2(mg, tmp_path, capsys):
    from structured_light_for_3d_model_replication_amd import ply
    from structured_light_for_3d_model_replication_amd import statistical_outlier_removal as sor
    P, C = _view()
    src, dst = str(tmp_path / "view.ply"), str(tmp_path / "clean.ply")
    ply.save_ply_open3d(P, C, src)
    assert sor.remove_outliers_keep_color2(src, dst) is None
    labels, info = co.dbscan_order_free(P, 5, 200)
    assert info["clusters"] == 2 and info["noise"] > 0
    keep = co.keep_largest_cluster(labels)
    assert 1400 < len(keep) < 1600  # the object, less a few tail points
    ind = co.remove_radius_outlier(P[keep], 5, 15)
    Q, Cq = ply.read_ply(dst)
    np.testing.assert_array_equal(Q, P[keep][ind])
    np.testing.assert_array_equal(Cq, C[keep][ind])
    assert capsys.readouterr().out == (f"Loading {src}...\n"
                                       f"Average point distance: {np.mean(co.nearest_neighbor_distance(P))}\n"
                                       "Clustering points...\n"
                                       "Removing outliers...\n"
                                       f"Cleaned points: {len(ind)}\n"
                                       f"Removed points: {len(keep) - len(ind)}\n"
                                       f"Saved cleaned cloud with colors to: {dst}\n")


def test_drop_in_recipe_1(mg, tmp_path, capsys):
    from structured_light_for_3d_model_replication_amd import ply
    from structured_light_for_3d_model_replication_amd import statistical_outlier_removal as sor
    P, C = _view()
    src, dst = str(tmp_path / "view.ply"), str(tmp_path / "clean.ply")
    ply.save_ply_open3d(P, C, src)
    assert sor.main([src, dst, "--recipe", "1"]) == 0
    ind, _ = merge_oracle.remove_statistical_outlier(P, 20, 2.0)
    Q, Cq = ply.read_ply(dst)
    np.testing.assert_array_equal(Q, P[ind])
    np.testing.assert_array_equal(Cq, C[ind])
    assert capsys.readouterr().out == (f"Loading {src}...\n"
                                       "Removing outliers...\n"
                                       f"Cleaned points: {len(ind)}\n"
                                       f"Removed points: {len(P) - len(ind)}\n"
                                       f"Saved cleaned cloud with colors to: {dst}\n")


def test_drop_in_without_colour_warns(mg, tmp_path, capsys):
    from structured_light_for_3d_model_replication_amd import statistical_outlier_removal as sor
    P, _ = _view()
    src, dst = tmp_path / "view.ply", str(tmp_path / "clean.ply")
    head = (f"ply\nformat ascii 1.0\nelement vertex {len(P)}\nproperty double x\nproperty double y\n"
            "property double z\nend_header\n")
    src.write_text(head + "".join(f"{x!r} {y!r} {z!r}\n" for x, y, z in P.tolist()))
    sor.remove_outliers_keep_color2(str(src), dst)
    assert "Warning: The input file does not have color data.\n" in capsys.readouterr().out
