"""Registration and ICP on the GPU (csrc/slreg.inl, the ICP and cell-grid code
of csrc/slmerge.hip) on the paths that well-behaved inputs never take, bit for
bit against oracle/registration_oracle.py and oracle/merge_oracle.py:

- the RANSAC walk over several batches of hypotheses and several chunks of
  validations, ending at the estimated k or at max_iteration, without the
  mutual filter, on its fallback, and on degenerate draws;
- the sparse cell table (a target grid of more than 2^26 cells: binary search)
  in RANSAC's validation and in ICP, and cells wider than the search radius;
- the radius search at the boundary between its LDS sort and its radix select,
  with ties across the cut;
- FPFH on duplicate points, collinear neighbours, zero normals and cut lists;
- feature matching on its single-kernel path, NaN and inf rows.

The inputs come from tests/registration_cases.py; tests/test_registration_
oracle.py proves on the CPU that each one reaches its branch.

Not covered, deliberately: the smaller validation chunk of a source of more
than 2^17 points (kVal * ns <= 2^25).  The oracle validates in a Python loop
over the source; enough validated hypotheses to fill such a chunk would take
it minutes."""
import numpy as np
import pytest

from oracle import merge_oracle as mo
from oracle import registration_oracle as ro
from tests import registration_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mg():
    from structured_light_for_3d_model_replication_amd import merge
    return merge


# ------------------------------------------------------------------ RANSAC ----
@pytest.mark.parametrize("name", rc.RANSAC_CASES)
def test_ransac_paths_vs_oracle(mg, name):
    """R1-R6 of tests/registration_cases.py: the transformation, fitness, RMSE,
    iterations, validations and correspondence count of the oracle's run with
    the same seed."""
    (S, T, FS, FT), kw = rc.ransac_case(name)
    want = rc.ransac_oracle(name)[0]
    args, kwargs = rc.gpu_kwargs(kw)
    got = mg.registration_ransac_based_on_feature_matching(S, T, FS, FT, *args, **kwargs)
    print(name, {k: got[k] for k in ("fitness", "inlier_rmse", "iterations", "validations", "correspondences")},
          "oracle", {k: want[k] for k in ("fitness", "inlier_rmse", "iterations", "validations")}, len(want["corres"]))
    np.testing.assert_array_equal(got["transformation"], want["transformation"])
    assert got["fitness"] == want["fitness"]
    assert got["inlier_rmse"] == want["inlier_rmse"]
    assert got["iterations"] == want["iterations"]
    assert got["validations"] == want["validations"]
    assert got["correspondences"] == len(want["corres"])


# --------------------------------------------------------------------- ICP ----
def _icp_equal(got, want):
    np.testing.assert_array_equal(got["transformation"], want["transformation"])
    assert got["fitness"] == want["fitness"]
    assert got["inlier_rmse"] == want["inlier_rmse"]
    assert got["iterations"] == want["iterations"]


@pytest.fixture(scope="module")
def icp_sheet(mg):
    """test_icp_known_motion_vs_oracle's sheet, motion, target and normals."""
    from tests.test_merge_oracle import _motion, _sheet
    S = _sheet(110, seed=3)
    M = _motion(2.0, [1.0, -0.7, 0.4])
    T = mo._transform(S, M)
    N = mg.estimate_normals(T, 6.0, 30).cpu().numpy()
    return S, M, T, N


@pytest.mark.parametrize("far", [2e4, 1e7])
def test_icp_sparse_cell_table_vs_oracle(mg, icp_sheet, far):
    """registration_icp on a target anchored at +-far: more than 2^26 cells, so
    k_icp_corr finds its cells by binary search (at 1e7 in cells of edge 20,
    wider than both distances) -- from the identity and from a near seed, the
    oracle's result on the same anchored input, and the motion recovered."""
    S, M, T, N = icp_sheet
    Ta = rc.with_anchors(T, far)
    Na = np.concatenate([N, [[0.0, 0.0, 1.0], [0.0, 1.0, 0.0]]])
    seed = M.copy()
    seed[:3, 3] += 0.3
    for max_dist, init, iters in ((5.0, None, 60), (1.0, seed, 30)):
        h, cells = rc.grid_cells(Ta, max_dist)
        assert cells > rc.DENSE_CELLS and h == (20.0 if far == 1e7 else max_dist)
        got = mg.registration_icp(S, Ta, Na, max_dist, init, max_iteration=iters)
        want = mo.registration_icp_point_to_plane(S, Ta, Na, max_dist, init, max_iteration=iters)
        print(far, max_dist, [(r["fitness"], r["inlier_rmse"], r["iterations"]) for r in (got, want)])
        _icp_equal(got, want)
        assert got["fitness"] > 0.9 and got["iterations"] >= 1
        if init is None:
            np.testing.assert_allclose(got["transformation"], M, atol=1e-6)


@pytest.mark.parametrize("far", [None, 2e4])
def test_icp_equidistant_targets_tie_to_the_lower_index(mg, far):
    """Source points exactly midway between two target points that lie in
    neighbouring cells and have different normals: the correspondence is the
    lower target index, whichever cell is scanned first (the targets are
    shuffled, so both orders occur) -- on the dense and on the sparse table."""
    (S, T, N), max_dist = rc.icp_ties(), 1.0
    if far is not None:
        T, N = rc.with_anchors(T, far), np.concatenate([N, [[0.0, 0.0, 1.0], [0.0, 1.0, 0.0]]])
    assert (rc.grid_cells(T, max_dist)[1] > rc.DENSE_CELLS) == (far is not None)
    corr, d2 = mo.icp_correspondences(S, T, max_dist)
    tied = [i for i in range(len(S)) if np.count_nonzero(((S[i] - T) ** 2).sum(axis=1) == d2[i]) == 2]
    lower_x_wins = sum(1 for i in tied if T[corr[i], 0] < S[i, 0])
    assert len(tied) > 100 and 50 < lower_x_wins < len(tied) - 50
    got = mg.registration_icp(S, T, N, max_dist, None, max_iteration=3)
    want = mo.registration_icp_point_to_plane(S, T, N, max_dist, None, max_iteration=3)
    print(far, [(r["fitness"], r["inlier_rmse"], r["iterations"]) for r in (got, want)])
    _icp_equal(got, want)
    assert got["fitness"] > 0.5 and got["iterations"] >= 1


# ----------------------------------------------------------- radius search ----
def _radius_equal(mg, name, max_nn):
    P, radius = rc.radius_case(name)
    idx, d2, cnt = (t.cpu().numpy() for t in mg.radius_search(P, radius, max_nn))
    wi, wd = rc.radius_oracle(name)
    for i in range(len(P)):
        k = min(len(wi[i]), max_nn)
        assert cnt[i] == k, f"{name} max_nn={max_nn} point {i}: count {cnt[i]} != {k}"
        np.testing.assert_array_equal(idx[i, :k], wi[i][:k], err_msg=f"{name} max_nn={max_nn} point {i}")
        np.testing.assert_array_equal(d2[i, :k], wd[i][:k], err_msg=f"{name} max_nn={max_nn} point {i}")


@pytest.mark.parametrize("name,max_nn", [
    ("c1024", 1024), ("c1024", 100),                     # exactly kNnCap candidates: the LDS sort at P = 1024
    ("c1025", 1024), ("c1025", 100), ("c1025", 1),       # one more: every row through the radix select
    ("identical", 1024),                                 # K == 0: the first 1024 indices
    ("lattice", 1024), ("lattice", 1000), ("lattice", 257),  # ties on d2 == K across the cut
    ("c1024_far", 1024), ("c1025_far", 100), ("identical_far", 1024), ("lattice_far", 1000),  # clamped cells
    ("n1", 10), ("n63", 10), ("n64", 64), ("n65", 100),
])
def test_radius_search_boundaries_vs_oracle(mg, name, max_nn):
    """(idx, d2, count) of every row == the oracle's ascending (d2, index)
    list cut at max_nn."""
    _radius_equal(mg, name, max_nn)


def test_radius_search_lattice_ties_straddle_the_cut():
    """(What makes the lattice cases a test of the index select: for every
    max_nn used above some query has equal d2 on both sides of the cut, and
    for 1024 and 1000 such a query overflows the LDS sort.)"""
    wi, wd = rc.radius_oracle("lattice")
    for max_nn in (1024, 1000, 257):
        assert any(len(d) > max_nn and d[max_nn - 1] == d[max_nn] for d in wd)
    for max_nn in (1024, 1000):
        assert any(len(d) > rc.NN_CAP and d[max_nn - 1] == d[max_nn] for d in wd)


# -------------------------------------------------------------------- FPFH ----
@pytest.mark.parametrize("max_nn", [100, 16])
def test_fpfh_degenerate_cloud_vs_oracle(mg, max_nn):
    """compute_fpfh_feature bit for bit on the cloud of duplicate points,
    collinear neighbours, zero normals and a clump whose lists are cut."""
    P, N = rc.fpfh_cloud()
    idx, d2 = ro.radius_neighbours(P, rc.FPFH_RADIUS, max_nn)
    assert any(np.any((d == 0.0) & (i != k)) for k, (i, d) in enumerate(zip(idx, d2)))
    assert any(len(i) == max_nn for i in idx)
    got = mg.compute_fpfh_feature(P, N, rc.FPFH_RADIUS, max_nn).cpu().numpy()
    want = ro.compute_fpfh(P, N, rc.FPFH_RADIUS, max_nn)
    assert np.isfinite(want).all() and want.any()
    np.testing.assert_array_equal(got, want)


# -------------------------------------------------------------- feature_nn ----
@pytest.mark.parametrize("na,nb", [(1, 1), (1, 65), (257, 64), (257, 65), (700, 64 * 15 + 1), (3, 0)])
def test_feature_nn_shapes_vs_oracle(mg, na, nb):
    """One kernel (at most 64 rows of B) and the split ranges, a last range of
    one row, no rows at all."""
    rng = np.random.default_rng(100 * na + nb)
    A, B = rng.normal(size=(na, 33)), rng.normal(size=(nb, 33))
    if nb:
        A[na // 2] = B[nb - 1]  # the last row of B is somebody's nearest
    want = ro.feature_nn(A, B)
    assert nb == 0 or want[na // 2] == nb - 1
    np.testing.assert_array_equal(mg.feature_nn(A, B).cpu().numpy(), want)


@pytest.mark.parametrize("nb", [40, 64 * 15 + 1])
def test_feature_nn_nan_inf_and_identical_rows(mg, nb):
    """A NaN query row -> -1; NaN everywhere in B -> all -1; rows holding
    +inf (a distance of inf or NaN never wins); every row of B equal ->
    index 0.  On the single-kernel path (nb = 40) and the split one."""
    rng = np.random.default_rng(nb)
    A, B = rng.normal(size=(300, 33)), rng.normal(size=(nb, 33))
    A[5] = np.nan
    A[6, 3] = np.nan
    A[7, 32] = np.inf
    A[8] = np.inf
    B[3, 0] = np.inf
    B[nb - 1] = np.inf
    B[10, 32] = np.nan
    want = ro.feature_nn(A, B)
    assert want[5] == -1 and want[6] == -1 and want[7] == -1 and want[8] == -1 and want[0] >= 0
    np.testing.assert_array_equal(mg.feature_nn(A, B).cpu().numpy(), want)
    want = ro.feature_nn(B, A)
    assert want[3] == -1 and want[10] == -1 and want[0] >= 0
    np.testing.assert_array_equal(mg.feature_nn(B, A).cpu().numpy(), want)
    nan_b = np.full((nb, 33), np.nan)
    np.testing.assert_array_equal(mg.feature_nn(A, nan_b).cpu().numpy(), np.full(300, -1))
    np.testing.assert_array_equal(ro.feature_nn(A, nan_b), np.full(300, -1))
    same = np.tile(B[1], (nb, 1))
    want = ro.feature_nn(A, same)
    assert np.array_equal(want[:5], np.zeros(5)) and want[5] == -1
    np.testing.assert_array_equal(mg.feature_nn(A, same).cpu().numpy(), want)


# --------------------------------------------------- non-finite coordinates ----
def _cube():
    return np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])


_NONFINITE = {
    "estimate_normals": ("non-finite point coordinates", lambda mg, bad, ok, F: mg.estimate_normals(bad, 1.0, 30)),
    "radius_search": ("non-finite point coordinates", lambda mg, bad, ok, F: mg.radius_search(bad, 1.0, 16)),
    "compute_fpfh_feature": ("non-finite point coordinates",
                             lambda mg, bad, ok, F: mg.compute_fpfh_feature(bad, np.tile([0.0, 0.0, 1.0], (8, 1)),
                                                                            1.0, 16)),
    "registration_icp": ("non-finite target coordinates",
                         lambda mg, bad, ok, F: mg.registration_icp(ok, bad, np.tile([0.0, 0.0, 1.0], (8, 1)), 1.0)),
    "registration_ransac_based_on_feature_matching": (
        "non-finite target coordinates",
        lambda mg, bad, ok, F: mg.registration_ransac_based_on_feature_matching(ok, bad, F[0], F[1], False, 1.0)),
    "remove_statistical_outlier": ("non-finite or degenerate point cloud",
                                   lambda mg, bad, ok, F: mg.remove_statistical_outlier(bad)),
}


@pytest.mark.parametrize("entry", list(_NONFINITE))
def test_nonfinite_coordinates_are_rejected(mg, entry):
    """The 8 corners of a unit cube with one coordinate +inf (in the target for
    ICP and RANSAC, whose 8 one-way correspondences reach the grid): every
    entry point that sorts a cloud into cells raises ValueError with its own
    message once the bounds are known, before any cell is keyed."""
    ok = _cube()
    bad = _cube()
    bad[5, 1] = np.inf
    F = np.random.default_rng(7).normal(size=(2, 8, 33))
    msg, call = _NONFINITE[entry]
    with pytest.raises(ValueError) as e:
        call(mg, bad, ok, F)
    assert str(e.value) == msg
