"""tests/cluster_oracle.py against itself: the sequential ClusterDBSCAN loop and
its order-free form give the same labels on every case the GPU tests use (that
is what justifies checking the GPU against the order-free form), scikit-learn
partitions the core points the same way, and keep-largest-cluster's tie and
all-noise behaviour."""
import numpy as np
import pytest

from tests import cluster_oracle as co


@pytest.mark.parametrize("name", sorted(co.CASES))
def test_two_forms_agree(name):
    s = co.solved(name)
    seq = co.dbscan_sequential(s["P"], s["eps"], s["min_points"], s["A"])
    np.testing.assert_array_equal(seq, s["labels"])
    assert seq.dtype == np.int32


def test_the_cases_hold_what_they_are_for():
    info = {k: co.solved(k)["info"] for k in co.CASES}
    assert info["single"] == {"clusters": 1, "core": 1, "noise": 0}
    assert info["fewer_than_min_points"] == {"clusters": 0, "core": 0, "noise": 7}
    assert info["min_points_one"]["noise"] == 0 and info["min_points_one"]["core"] == 500
    assert info["identical"] == {"clusters": 1, "core": 300, "noise": 0}
    assert (co.solved("one_ball")["counts"] == 5000).all() and info["one_ball"]["clusters"] == 1
    assert (co.solved("lattice_closed")["counts"] == 1).all() and info["lattice_closed"]["noise"] == 120
    assert co.solved("lattice_open")["counts"].min() == 4 and info["lattice_open"] == {"clusters": 1, "core": 120,
                                                                                      "noise": 0}
    assert info["helix"]["clusters"] == 1 and info["helix"]["noise"] == 0
    d = co.solved("dense_cell")
    assert d["info"]["clusters"] >= 2 and d["info"]["noise"] > 0
    sizes = np.bincount(d["labels"][d["labels"] >= 0])
    assert sizes[0] >= 2999 and sizes.max() > sizes[0] and sizes.argmax() > 0  # the largest is not the first
    assert info["wide_extent"]["clusters"] == 2
    b = info["blobs_and_noise"]
    assert b["clusters"] > 2 and b["core"] > 0 and b["noise"] > 0
    lab = co.solved("blobs_and_noise")["labels"]
    assert (lab >= 0).sum() > b["core"]  # border points


@pytest.mark.parametrize("order", ["a", "b"])
def test_bridge_is_a_contested_border_point(order):
    P, eps, mp, bridge = co.bridge_rows(order)
    A = co.adjacency(P, eps)
    labels, info = co.dbscan_order_free(P, eps, mp, A)
    cnt = co.counts_of(A)
    assert cnt[bridge] == 3 and info["core"] == 16 and info["clusters"] == 2
    nb = A.indices[A.indptr[bridge]:A.indptr[bridge + 1]]
    nb = nb[cnt[nb] >= mp]
    assert sorted(labels[nb]) == [0, 1]
    assert labels[bridge] == 0
    np.testing.assert_array_equal(co.dbscan_sequential(P, eps, mp, A), labels)


def test_sequential_marks_the_bridge_noise_first():
    # order "a": index 0 is the bridge, not core, so the loop labels it noise before any cluster exists
    P, eps, mp, bridge = co.bridge_rows("a")
    assert bridge == 0 and co.counts_of(co.adjacency(P, eps))[0] < mp


@pytest.mark.parametrize("seed,n,eps,mp", [(0, 400, 0.9, 5), (1, 1500, 1.2, 10), (2, 64, 1.5, 3)])
def test_core_partition_matches_sklearn(seed, n, eps, mp):
    cluster = pytest.importorskip("sklearn.cluster")
    P = np.random.default_rng(seed).uniform(0, 10, (n, 3))  # random doubles: no distance equals eps
    labels, _ = co.dbscan_order_free(P, eps, mp)
    # scikit-learn's radius test is d <= eps; on these inputs no distance equals eps
    sk = cluster.DBSCAN(eps=eps, min_samples=mp, algorithm="brute").fit(P)
    core = np.zeros(n, dtype=bool)
    core[sk.core_sample_indices_] = True
    np.testing.assert_array_equal(core, co.radius_count(P, eps) >= mp)
    assert core.any()
    np.testing.assert_array_equal(labels < 0, sk.labels_ < 0)
    # the same partition of the core points (both number clusters by first core index)
    np.testing.assert_array_equal(labels[core], sk.labels_[core])


def test_keep_largest_cluster():
    s = co.solved("equal_twins")
    sizes = np.bincount(s["labels"][s["labels"] >= 0])
    assert len(sizes) >= 2 and sizes[0] == sizes[1] == sizes.max()
    np.testing.assert_array_equal(co.keep_largest_cluster(s["labels"]), np.nonzero(s["labels"] == 0)[0])
    np.testing.assert_array_equal(co.keep_largest_cluster(np.array([1, 1, 0, -1, -1, -1])), [0, 1])
    np.testing.assert_array_equal(co.keep_largest_cluster(np.array([1, 0, 0, 1, -1])), [1, 2])   # tie: lowest label
    np.testing.assert_array_equal(co.keep_largest_cluster(np.array([-1, -1, -1])), [0, 1, 2])    # all noise
    assert len(co.keep_largest_cluster(np.zeros(0, np.int32))) == 0


def test_radius_filter_and_nn_distance():
    P = np.array([[0.0, 0, 0], [0.5, 0, 0], [0.9, 0, 0], [5.0, 0, 0], [5.0, 0, 0]])
    np.testing.assert_array_equal(co.radius_count(P, 0.5), [1, 2, 2, 2, 2])  # 0.5 apart: not neighbours
    np.testing.assert_array_equal(co.radius_count(P, 1.0, cap=2), [2, 2, 2, 2, 2])
    np.testing.assert_array_equal(co.remove_radius_outlier(P, 2, 1.0), [0, 1, 2])
    np.testing.assert_array_equal(co.nearest_neighbor_distance(P), [0.5, 0.4, 0.4, 0.0, 0.0])
    np.testing.assert_array_equal(co.nearest_neighbor_distance(P[:1]), [0.0])
    with pytest.raises(ValueError, match="number of points and radius must be positive"):
        co.remove_radius_outlier(P, 0, 1.0)
