"""The global-registration oracle (oracle/registration_oracle.py) on its own,
CPU only: the fdlibm atan2 against libm, the 3x3 Jacobi SVD against LAPACK,
Umeyama on exact rigid motions, FPFH's invariance under rigid motion, the
feature matching and RANSAC recovering a known motion.  (Parity with Open3D is
unpinned: it is not in this image.)"""
import math

import numpy as np

from oracle import merge_oracle as mo
from oracle import registration_oracle as ro
from tests import registration_cases as rc
from tests.registration_cases import _rot, blob  # noqa: F401  (the other test modules import them from here)


def test_atan2_within_one_ulp_of_libm():
    rng = np.random.default_rng(1)
    for _ in range(20000):
        y, x = rng.normal(size=2) * 10.0 ** rng.uniform(-6, 6, size=2)
        a, b = ro.atan2_det(y, x), math.atan2(y, x)
        assert abs(a - b) <= math.ulp(b), (y, x)
    for y, x in [(0.0, -1.0), (-0.0, -1.0), (1.0, 0.0), (-1.0, 0.0), (0.0, 0.0), (-0.0, 0.0), (1.0, 1.0),
                 (1e-300, -1.0), (1e300, 1e-300), (-2.0, 1.0)]:
        assert ro.atan2_det(y, x) == math.atan2(y, x), (y, x)


def test_jacobi_svd3_against_lapack():
    rng = np.random.default_rng(2)
    for k in range(300):
        A = rng.normal(size=(3, 3)) * 10.0 ** rng.uniform(-3, 3)
        if k % 7 == 0:
            A[:, 2] = A[:, 0] + A[:, 1]  # rank 2
        U, s, V = ro.jacobi_svd3(A.tolist())
        U, V, s = np.array(U), np.array(V), np.array(s)
        ref = np.linalg.svd(A, compute_uv=False)
        np.testing.assert_allclose(s, ref, rtol=1e-12, atol=1e-12 * ref[0])
        np.testing.assert_allclose(U @ np.diag(s) @ V.T, A, atol=1e-12 * ref[0])
        np.testing.assert_allclose(U.T @ U, np.eye(3), atol=1e-13)
        np.testing.assert_allclose(V.T @ V, np.eye(3), atol=1e-13)
    U, s, V = ro.jacobi_svd3([[0.0] * 3] * 3)
    assert s == [0.0, 0.0, 0.0] and U == [[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]


def test_umeyama_recovers_rigid_motion():
    rng = np.random.default_rng(3)
    for _ in range(200):
        R = _rot(*rng.uniform(-math.pi, math.pi, size=3))
        t = rng.normal(size=3) * 50
        S = rng.normal(size=(3, 3)) * 30
        D = S @ R.T + t
        M = np.array(ro.umeyama3(S.tolist(), D.tolist()))
        np.testing.assert_allclose(M[:3, :3], R, atol=1e-9)
        np.testing.assert_allclose(M[:3, 3], t, atol=1e-7)
        assert np.linalg.det(M[:3, :3]) > 0


def test_radius_neighbours_sorted_and_capped():
    P = blob(400, seed=4)
    idx, d2 = ro.radius_neighbours(P, 12.0, 10)
    for i in range(len(P)):
        assert idx[i][0] == i and d2[i][0] == 0.0  # itself first
        assert len(idx[i]) <= 10
        assert np.all(np.diff(d2[i]) >= 0)
        assert np.all(d2[i] < 144.0)


def test_fpfh_invariant_under_rigid_motion():
    P = blob(900, seed=5)
    N = mo.estimate_normals(P, 8.0, 30)
    F = ro.compute_fpfh(P, N, 20.0, 100)
    R = _rot(0.3, -0.2, 0.5)
    Q = P @ R.T + np.array([10.0, -4.0, 7.0])
    NQ = N @ R.T  # the same normals moved (estimate_normals' eigenvector signs are arbitrary)
    FQ = ro.compute_fpfh(Q, NQ, 20.0, 100)
    assert F.shape == (900, 33)
    np.testing.assert_allclose(F.sum(axis=1), FQ.sum(axis=1), rtol=1e-6, atol=1e-6)
    for k in range(3):  # every third sums to 200 (the SPFH's 100 plus the weighted neighbours' 100)
        np.testing.assert_allclose(F[:, 11 * k:11 * k + 11].sum(axis=1), 200.0, rtol=1e-9)
    assert np.mean(np.abs(F - FQ)) < 1.0  # rounding can move a pair across a bin edge, rarely


def test_feature_nn_order_and_ties():
    rng = np.random.default_rng(6)
    A = rng.normal(size=(50, 33))
    B = np.concatenate([A[::-1], A[:5]])  # duplicates: ties to the lower index
    nn = ro.feature_nn(A, B)
    np.testing.assert_array_equal(nn, np.arange(49, -1, -1))
    d = ro.feature_dist2(A[0], B)
    assert d[49] == 0.0 and d[50] == 0.0 and nn[0] == 49


def test_ransac_recovers_motion():
    P = blob(800, seed=7)
    N = mo.estimate_normals(P, 8.0, 30)
    F = ro.compute_fpfh(P, N, 20.0, 100)
    R = _rot(0.0, 0.35, 0.0)
    t = np.array([12.0, 0.0, -5.0])
    Q = P @ R.T + t
    NQ = mo.estimate_normals(Q, 8.0, 30)
    FQ = ro.compute_fpfh(Q, NQ, 20.0, 100)
    res = ro.ransac_based_on_feature_matching(P, Q, F, FQ, 6.0, seed=11)
    M = res["transformation"]
    assert res["fitness"] > 0.9 and res["validations"] >= 1 and res["iterations"] >= 1
    np.testing.assert_allclose(M[:3, :3], R, atol=1e-6)
    np.testing.assert_allclose(M[:3, 3], t, atol=1e-4)
    # the same seed: the same run; another seed may stop elsewhere but is just as good
    res2 = ro.ransac_based_on_feature_matching(P, Q, F, FQ, 6.0, seed=11)
    assert res2["iterations"] == res["iterations"] and np.array_equal(res2["transformation"], M)


def test_ransac_degenerate_inputs():
    P = blob(50, seed=8)
    F = np.zeros((50, 33))
    res = ro.ransac_based_on_feature_matching(P[:2], P[:2], F[:2], F[:2], 5.0)
    assert res["iterations"] == 0 and np.array_equal(res["transformation"], np.eye(4))
    res = ro.ransac_based_on_feature_matching(P, P, F, F, 0.0)  # max_correspondence_distance <= 0
    assert res["iterations"] == 0 and np.array_equal(res["transformation"], np.eye(4))
    # all features equal: every source point matches target 0, one-way (no mutual pairs beyond one)
    c = ro.correspondences_from_features(F, F, True)
    np.testing.assert_array_equal(c[:, 1], 0)


# ---- the scenarios of tests/registration_cases.py reach their branches ----
# (tests/test_gpu_registration_paths.py compares the GPU with the oracle on the
# same scenarios; what is asserted here is what makes each one reach the code
# it is meant for.  Oracle times: this suite's CPU, one thread.)

def test_trace_leaves_the_result_unchanged():
    """ransac_based_on_feature_matching(trace=[...]) returns what the run
    without a trace returns; one record per iteration, flag 2 per validation."""
    inputs, kw = rc.ransac_case("r1_p10")
    plain = ro.ransac_based_on_feature_matching(*inputs, **kw)
    traced, trace, _ = rc.ransac_oracle("r1_p10")
    assert set(plain) == set(traced)
    for k in plain:
        np.testing.assert_array_equal(plain[k], traced[k], err_msg=k)
    assert len(trace) == plain["iterations"]
    assert sum(1 for f, _ in trace if f == 2) == plain["validations"]
    nc = len(plain["corres"])
    assert all(f in (0, 1, 2) and len(c) == 3 and all(0 <= x < nc for x in c) for f, c in trace)
    assert trace[7][1] == tuple(ro.draw(kw["seed"], 21 + j, nc) for j in range(3))


def test_r1_stops_at_est_k_after_many_batches():
    """R1: one-way correspondences with 7 % / 10 % inliers and the reference's
    settings run for 55 259 / 13 489 iterations (102 / 39 validations; 0.45 s /
    0.2 s of oracle): more than one batch of 4096 hypotheses, the last one
    partial, stopped by the estimated k and not by max_iteration."""
    for name in ("r1_p07", "r1_p10"):
        res, trace, _ = rc.ransac_oracle(name)
        kw = rc.ransac_case(name)[1]
        assert kw["mutual_filter"] is False and (kw["edge_sim"], kw["max_iteration"], kw["confidence"]) == \
            (0.9, 100000, 0.999)
        assert rc.BATCH < res["iterations"] < kw["max_iteration"], name
        assert res["iterations"] % rc.BATCH != 0, name
        assert res["validations"] >= 1 and res["fitness"] > 0.9, name


def test_r2_fills_several_validation_chunks_in_one_batch():
    """R2: edge similarity 0.5, confidence 1 (est_k never shrinks while the
    inlier ratio is below 1), 5000 iterations on 150 points: the first batch
    holds 1012 validated hypotheses -- three full chunks of 256 and one of
    244 -- and the run ends at max_iteration (1239 validations; the oracle
    takes 2.7 s)."""
    res, trace, _ = rc.ransac_oracle("r2")
    assert res["iterations"] == 5000 == rc.ransac_case("r2")[1]["max_iteration"]
    passes = rc.batch_passes(trace)
    assert any(p > 2 * rc.VAL_CHUNK and p % rc.VAL_CHUNK != 0 for p in passes), passes
    assert sum(passes) == res["validations"]


def test_r3_runs_to_each_iteration_cap():
    """R3: confidence 1 and max_iteration 1 / 4096 / 4097: a single hypothesis,
    exactly one batch, one batch and one hypothesis."""
    for cap in rc.R3_CAPS:
        res, trace, _ = rc.ransac_oracle(f"r3_{cap}")
        assert res["iterations"] == cap == len(trace)
    assert rc.ransac_oracle(f"r3_{rc.BATCH}")[0]["validations"] >= 1


def test_r4_validates_degenerate_draws():
    """R4: five correspondences, 300 iterations: validated hypotheses whose
    three draws hold the same correspondence twice (a rank-1 covariance in
    Umeyama) and three times (a zero one), and the run ends at max_iteration."""
    res, trace, _ = rc.ransac_oracle("r4")
    assert len(res["corres"]) == 5 and res["iterations"] == 300
    distinct = [len(set(c)) for f, c in trace if f == 2]
    assert distinct.count(2) >= 1 and distinct.count(1) >= 1 and distinct.count(3) >= 1
    assert 0.0 < res["fitness"] < 1.0


def test_r5_falls_back_to_the_one_way_set():
    """R5: fewer mutual pairs than a tenth of the source: the correspondences
    are the one-way set, a pair for every row that has a neighbour."""
    (S, T, FS, FT), kw = rc.ransac_case("r5")
    ij, ji = ro.feature_nn(FS, FT), ro.feature_nn(FT, FS)
    mutual = sum(1 for i, j in enumerate(ij) if j >= 0 and ji[j] == i)
    with_neighbour = int(np.count_nonzero(ij >= 0))
    assert kw["mutual_filter"] is True
    assert mutual < int(np.float32(0.1) * np.float32(len(S)))
    assert len(ro.correspondences_from_features(FS, FT, True)) == with_neighbour > mutual
    assert with_neighbour == len(S) - 1  # (the NaN row)
    res, trace, _ = rc.ransac_oracle("r5")
    assert len(res["corres"]) == with_neighbour and res["validations"] >= 1


def test_r6_grids_are_sparse_and_anchors_change_nothing():
    """R6: the anchored target's grid, counted as make_grid counts it, has
    more than 2^26 cells (the sparse cell table); at 1e7 with max_dist 1 the
    cell edge is the clamp extent / 1e6 = 20 > max_dist.  The anchors have NaN
    features and are far from everything: the 2e4 run equals the plain one."""
    (S, T, FS, FT), kw = rc.ransac_case("r6_2e4")
    h, cells = rc.grid_cells(T, kw["max_dist"])
    assert h == kw["max_dist"] == 2.0 and cells > rc.DENSE_CELLS
    assert rc.grid_cells(rc.ransac_case("r1_p10")[0][1], 2.0)[1] <= rc.DENSE_CELLS
    plain, far = rc.ransac_oracle("r1_p10")[0], rc.ransac_oracle("r6_2e4")[0]
    for k in plain:
        np.testing.assert_array_equal(plain[k], far[k], err_msg=k)
    (S, T, FS, FT), kw = rc.ransac_case("r6_1e7")
    h, cells = rc.grid_cells(T, kw["max_dist"])
    assert kw["max_dist"] == 1.0 and h == 20.0 and cells > rc.DENSE_CELLS
    res = rc.ransac_oracle("r6_1e7")[0]
    assert res["iterations"] > rc.BATCH and res["validations"] >= 1


def test_radius_clouds_reach_the_sort_and_the_select():
    """The radius-search clouds: every query of the 1024-point cluster has
    exactly 1024 candidates (the LDS sort's capacity), of the 1025-point one
    1025 (the radix select), 1500 for the identical points, all at d2 == 0;
    the lattice has queries on both sides with integer d2, and for each
    max_nn a query whose max_nn-th and next smallest d2 are equal."""
    for name, n in (("c1024", 1024), ("c1025", 1025), ("identical", 1500)):
        idx, d2 = rc.radius_oracle(name)
        assert len(idx) == n and all(len(i) == n for i in idx), name
    assert rc.NN_CAP == 1024 and all(not d.any() for d in rc.radius_oracle("identical")[1])
    idx, d2 = rc.radius_oracle("lattice")
    counts = np.array([len(i) for i in idx])
    assert counts.min() <= rc.NN_CAP < counts.max()
    for max_nn in (1024, 1000, 257):
        assert any(len(d) > max_nn and d[max_nn - 1] == d[max_nn] for d in d2), max_nn
    P, radius = rc.radius_case("c1025_far")
    assert rc.grid_cells(P, radius)[0] == 20.0 > radius


def test_fpfh_cloud_holds_every_degenerate_ingredient():
    """The FPFH cloud: rows with a d2 == 0 neighbour other than themselves,
    rows cut at max_nn (100 and 16), pairs along a normal and zero normals
    (both: a zero cross product), a count that straddles the 64-point
    workgroup."""
    P, N = rc.fpfh_cloud()
    assert 1100 <= len(P) <= 1300 and len(P) % 64 != 0
    for max_nn in (100, 16):
        idx, d2 = ro.radius_neighbours(P, rc.FPFH_RADIUS, max_nn)
        assert any(np.any((d == 0.0) & (i != k)) for k, (i, d) in enumerate(zip(idx, d2)))
        assert any(len(i) == max_nn for i in idx) and any(1 < len(i) < max_nn for i in idx)
    assert np.count_nonzero(~N.any(axis=1)) == 100
    line = slice(135, 235)
    for a, b in ((135, 136), (200, 150), (234, 135)):
        assert ro._norm3(ro._cross3(tuple(P[b] - P[a]), tuple(N[a]))) == 0.0
        assert ro.pair_features(P[a], N[a], P[b], N[b]) == (0.0, 0.0, 0.0, 0.0)
    np.testing.assert_array_equal(N[line], np.tile(N[135], (100, 1)))


def test_icp_ties_put_the_lower_index_in_either_cell():
    """The ICP tie scenario: 552 source points have exactly two nearest
    targets at the same d2, in neighbouring cells of edge 1 (integer x); the
    oracle takes the lower index, which is the lower-x cell for about half."""
    from oracle import merge_oracle as mo
    S, T, N = rc.icp_ties()
    corr, d2 = mo.icp_correspondences(S, T, 1.0)
    assert (corr >= 0).all() and np.all(d2 == 0.265625)
    tied = [i for i in range(len(S)) if np.count_nonzero(((S[i] - T) ** 2).sum(axis=1) == d2[i]) == 2]
    assert len(tied) == 24 * 23
    for i in tied:
        pair = np.flatnonzero(((S[i] - T) ** 2).sum(axis=1) == d2[i])
        assert corr[i] == pair.min() and abs(T[pair[0], 0] - T[pair[1], 0]) == 1.0
        assert not np.array_equal(N[pair[0]], N[pair[1]])
    lower_x = sum(1 for i in tied if T[corr[i], 0] < S[i, 0])
    assert 200 < lower_x < len(tied) - 200
