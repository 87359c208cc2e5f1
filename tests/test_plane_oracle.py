"""tests/plane_oracle.py -- the CPU restatement of the plane RANSAC
(sl_segment_plane, csrc/slplane.inl) -- does what a background removal needs.
Open3D is not installed: parity with Open3D is unpinned, and these tests check
the restatement's own properties (the GPU is checked against it bit for bit in
test_gpu_background.py), and that every input of tests/plane_cases.py reaches
the path of slplane.inl it is named for (the GPU is checked on those in
test_gpu_plane_paths.py)."""
import math

import numpy as np
import pytest

from tests import plane_cases as pc
from tests import plane_oracle as po


@pytest.fixture(scope="module")
def wall():
    P, is_wall = po.wall_scene()  # default_rng(1), n = 20000, 60 % wall
    model, inl, it = po.segment_plane(P, 10.0, 3, 1000, seed=7)
    return P, is_wall, model, inl, it


def test_wall_scene_exits_early(wall):
    assert wall[4] < 1000


def test_wall_scene_takes_no_object_point(wall):
    _, is_wall, _, inl, _ = wall
    assert is_wall[inl].all()


def test_wall_scene_takes_the_wall(wall):
    _, is_wall, _, inl, _ = wall
    assert is_wall[inl].sum() >= 0.95 * is_wall.sum()


def test_wall_scene_refined_normal(wall):
    n = wall[2][:3]
    assert np.abs(np.abs(n) - np.array([0.0, 0.0, 1.0])).max() < 1e-2
    assert abs(np.linalg.norm(n) - 1.0) < 1e-12


def test_inliers_ascending(wall):
    inl = wall[3]
    assert (np.diff(inl) > 0).all()


def test_same_seed_same_result_other_seed_other_draw(wall):
    P, _, model, inl, it = wall
    m2, i2, it2 = po.segment_plane(P, 10.0, 3, 1000, seed=7)
    assert np.array_equal(m2, model) and np.array_equal(i2, inl) and it2 == it
    n = len(P)
    assert [po.draw(7, k, n) for k in range(30)] != [po.draw(8, k, n) for k in range(30)]
    assert all(0 <= po.draw(8, k, n) < n for k in range(1000))


@pytest.mark.parametrize("n", [1, 255, 4096, 4097, 10001])
def test_ordered_sum_vs_fsum(n):
    v = np.random.default_rng(n).uniform(0.0, 10.0, n)
    exact = math.fsum(v)
    assert abs(po.ordered_sum(v) - exact) <= 1e-12 * abs(exact)


def test_ordered_sum_is_the_stated_order():
    # lane l of chunk c holds rows 4096 c + 256 r + l; the tree pairs l with l + s
    v = np.random.default_rng(5).uniform(-1.0, 1.0, 4096 + 300)
    pad = np.zeros(8192)
    pad[: len(v)] = v
    tot = 0.0
    for c in range(2):
        a = [0.0] * 256
        for lane in range(256):
            for r in range(16):
                a[lane] = a[lane] + float(pad[4096 * c + 256 * r + lane])
        s = 128
        while s:
            for lane in range(s):
                a[lane] = a[lane] + a[lane + s]
            s //= 2
        tot = tot + a[0]
    assert po.ordered_sum(v) == tot


def test_scatter_runs_every_iteration():
    _, _, it = po.segment_plane(po.scatter_scene(4099), 2.0, 3, 300, seed=7)
    assert it == 300


def test_collinear_gives_zero_plane():
    P = np.outer(np.arange(50.0), [1.0, 2.0, 3.0])
    model, inl, it = po.segment_plane(P, 1.0, 3, 50, seed=1)
    assert np.array_equal(model, np.zeros(4)) and len(inl) == 0 and it == 50


def test_bad_arguments():
    P = po.scatter_scene(10)
    with pytest.raises(ValueError):
        po.segment_plane(P, 1.0, 2, 10)
    with pytest.raises(ValueError):
        po.segment_plane(P[:2], 1.0, 3, 10)
    with pytest.raises(ValueError):
        po.segment_plane(po.scatter_scene(40), 1.0, 17, 10)


# ---- tests/plane_cases.py: every case reaches the path it is named for ----
# (the GPU is compared with the oracle on the same cases in test_gpu_plane_paths.py)
def _chunks(n):
    return (n + po.CHUNK - 1) // po.CHUNK


def test_every_case_is_deterministic_and_listed():
    assert len(set(pc.CASES)) == len(pc.CASES) == 23
    assert set(pc.BATCH_CASES) | set(pc.TIE_CASES) <= set(pc.CASES)
    for name in ("layers_jitter_late", "strict_closed", "nonfinite"):
        P, kw = pc.case(name)
        Q, kw2 = pc._CASES[name]()
        assert kw == kw2 and np.array_equal(P, Q, equal_nan=True)


@pytest.mark.parametrize("name, late", [("layers_jitter_late", True), ("layers_jitter_early", False)])
def test_case_layers_jitter_has_more_than_256_ties(name, late):
    P, kw = pc.case(name)
    _, inl, it = pc.oracle(name)
    idx, rmse, planes = pc.ties(name)
    assert len(P) == 288 and 256 * 64 < it < kw["num_iterations"] and len(inl) == 24
    assert len(rmse) > 256
    win = int(np.argmin(rmse))
    assert win >= 256 if late else win < 256
    assert (np.delete(rmse, win) > rmse[win]).all()  # strictly the least: no tie on rmse
    np.testing.assert_array_equal(np.nonzero(po.distances(P, planes[win]) < 1.0)[0], inl)
    if not late:
        # a comparison that starts afresh in the second group of 256 would end on another layer
        other = planes[256 + int(np.argmin(rmse[256:]))]
        assert not np.array_equal(np.nonzero(po.distances(P, other) < 1.0)[0], inl)


def test_case_layers_jitter_late_discriminates():
    """WRONG VARIANT: the best among the first 256 ties only (the later groups
    of k_plane_err ignored) keeps another layer."""
    P, _ = pc.case("layers_jitter_late")
    _, inl, _ = pc.oracle("layers_jitter_late")
    _, rmse, planes = pc.ties("layers_jitter_late")
    wrong = planes[int(np.argmin(rmse[:256]))]
    wrong_inl = np.nonzero(po.distances(P, wrong) < 1.0)[0]
    assert len(wrong_inl) == len(inl) and not np.array_equal(wrong_inl, inl)


def test_case_layers_exact_every_tie_has_rmse_zero():
    P, _ = pc.case("layers_exact")
    _, inl, _ = pc.oracle("layers_exact")
    _, rmse, planes = pc.ties("layers_exact")
    assert len(rmse) > 256 and (rmse == 0.0).all()
    layer = [np.nonzero(po.distances(P, pl) < 1.0)[0] for pl in planes]
    np.testing.assert_array_equal(layer[0], inl)  # the earliest tie stays the winner
    assert len(set(P[inl, 2])) == 1
    others = [j for j in range(256, len(layer)) if not np.array_equal(layer[j], inl)]
    assert others
    # WRONG VARIANT: a later tie with an equal rmse replaces the winner (<= for <)
    best, best_rmse = 0, rmse[0]
    for j in range(1, len(rmse)):
        if rmse[j] <= best_rmse:
            best, best_rmse = j, rmse[j]
    assert best == len(rmse) - 1 and not np.array_equal(layer[best], inl)
    # ... and so does a rule that restarts at each group of 256 ((j == 0) for (g == 0 && j == 0))
    assert not np.array_equal(layer[256], inl)


def test_case_scatter_1000_wins_late():
    P, kw = pc.case("scatter_1000")
    assert pc.oracle("scatter_1000")[2] == 1000
    idx, rmse, _ = pc.ties("scatter_1000")
    assert idx[int(np.argmin(rmse))] >= 300
    # the helpers with explicit arguments say the same as the cached ones
    args = (P, kw["distance_threshold"], kw["ransac_n"], kw["num_iterations"], kw["probability"], kw["seed"])
    assert pc.tie_report(*args) == tuple(rmse) and len(rmse) == 2
    assert pc.winning_iteration(*args) == idx[int(np.argmin(rmse))]


def test_case_wall30_stops_inside_a_large_batch():
    assert 256 < pc.oracle("wall30")[2] < 1000


def test_case_wall_1m_has_257_chunks():
    P, _ = pc.case("wall_1m")
    _, inl, it = pc.oracle("wall_1m")
    assert _chunks(len(P)) == 257 and 0 < it < 64
    assert inl[-1] >= 256 * po.CHUNK  # the only point of the last chunk is an inlier
    assert len(inl) > 0.85 * len(P)


@pytest.mark.parametrize("name, branch", [("wall_x", "x"), ("wall_y", "y"), ("lattice_x", "x"), ("lattice_y", "y")])
def test_case_fit_takes_the_other_branches(name, branch):
    P, _ = pc.case(name)
    _, inl, _ = pc.oracle(name)
    assert pc.fit_branch(P, inl) == branch
    det = pc.fit_determinants(P, inl)
    if name.startswith("lattice"):
        assert sum(d == 0.0 for d in det) == 2 and len(inl) == 289  # the strict > decides between 0 and 0
    else:
        assert len(inl) > 0.55 * len(P)


def test_case_wall_diag_determinants_nearly_equal():
    P, _ = pc.case("wall_diag")
    model, inl, _ = pc.oracle("wall_diag")
    det = np.array(pc.fit_determinants(P, inl))
    assert det.max() / det.min() < 1.01 and len(inl) > 0.55 * len(P)
    assert np.abs(np.abs(model[:3]) - 1.0 / math.sqrt(3.0)).max() < 1e-3


@pytest.mark.parametrize("name, rn", [("rn4", 4), ("rn16", 16), ("rn16_n16", 16)])
def test_case_ransac_n_ends(name, rn):
    P, kw = pc.case(name)
    model, inl, it = pc.oracle(name)
    assert kw["ransac_n"] == rn and len(inl) > 0 and np.isfinite(model).all() and 1 <= it <= 1000
    if name == "rn16_n16":
        assert len(P) == 16


@pytest.mark.parametrize("name", ["rn16_low_fitness_2", "rn16_low_fitness_20"])
def test_case_rn16_low_fitness_stops_after_the_first_inlier(name):
    P, kw = pc.case(name)
    _, inl, it = pc.oracle(name)
    fitness = len(inl) / len(P)
    assert 0.0 < fitness < 0.1
    p = math.pow(fitness, 16.0)
    assert p > 0.0 and 1.0 - p == 1.0 and math.log(1.0 - p) == 0.0  # k = log(1 - probability) / 0 = -inf
    first = pc.first_valid(P, 16, kw["seed"], with_inlier_below=kw["distance_threshold"])
    assert it == first + 1 and it < 300 // 10


def test_case_flat_reaches_fitness_one():
    P, kw = pc.case("flat")
    _, inl, it = pc.oracle("flat")
    np.testing.assert_array_equal(inl, np.arange(81))
    assert it == pc.first_valid(P, 3, kw["seed"]) + 1 < 100


def test_case_zero_iterations():
    model, inl, it = pc.oracle("zero_iterations")
    assert np.array_equal(model, np.zeros(4)) and len(inl) == 0 and it == 0


def test_case_strict_threshold_meets_distances_equal_to_it():
    P, kw = pc.case("strict_closed")
    ids = [po.draw(kw["seed"], k, len(P)) for k in range(3)]
    assert (P[ids, 2] == 1.0).all()
    pl = po.hypothesis(P, kw["seed"], 0, 3)
    assert np.array_equal(np.abs(pl), [0.0, 0.0, 1.0, 1.0]) and pl[2] == -pl[3]
    dist = po.distances(P, pl)
    assert (dist == 1.0).sum() == 578 and (dist == 0.0).sum() == 289
    _, closed, it = pc.oracle("strict_closed")
    np.testing.assert_array_equal(closed, np.nonzero(P[:, 2] == 1.0)[0])
    assert it == 1
    Po, kwo = pc.case("strict_open")
    assert np.array_equal(P, Po) and kwo["distance_threshold"] > 1.0 and kwo["seed"] == kw["seed"]
    _, opened, it = pc.oracle("strict_open")
    np.testing.assert_array_equal(opened, np.arange(867))
    assert it == 1
    # WRONG VARIANT: the threshold as <= takes the other two layers at threshold 1.0
    assert (dist <= kw["distance_threshold"]).sum() == 867 != len(closed)


def test_case_nonfinite_points_are_never_inliers():
    P, kw = pc.case("nonfinite")
    bad = pc.nonfinite_indices()
    assert len(set(bad)) == 5 and sorted(np.nonzero(~np.isfinite(P).all(1))[0]) == sorted(bad)
    assert np.isnan(P).any() and (P == np.inf).any() and (P == -np.inf).any()
    assert (~np.isfinite(P)).sum() == 5
    model, inl, it = pc.oracle("nonfinite")
    assert np.isfinite(model).all() and not set(bad) & set(inl.tolist()) and len(inl) > 0.55 * len(P)
    # iterations 0, 1 and 2 sample a NaN, a +inf and a -inf point, and the walk ran them
    assert it >= 3
    for i in range(3):
        ids = [po.draw(kw["seed"], 3 * i + k, len(P)) for k in range(3)]
        assert set(ids) & set(bad[:3])
        with np.errstate(all="ignore"):
            pl = po.hypothesis(P, kw["seed"], i, 3)
            near = po.distances(P, pl) < np.inf
        # valid (its length is not 0.0), and no point is within any threshold of it
        assert pl is not None and np.isnan(pl).any() and not near.any()


@pytest.mark.parametrize("n", [4096, 8192])
def test_case_full_chunks_have_no_padding(n):
    P, _ = pc.case(f"full_chunks_{n}")
    _, inl, it = pc.oracle(f"full_chunks_{n}")
    assert len(P) == n and n % po.CHUNK == 0 and it < 1000 and len(inl) > 0.55 * n
