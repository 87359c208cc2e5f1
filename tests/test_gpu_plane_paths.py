"""Plane segmentation on the GPU (sl_segment_plane, csrc/slplane.inl) on the
paths that a wall behind an object never takes, bit for bit against
tests/plane_oracle.py -- plane_model, inliers, iterations and the rest:

- more than 256 hypotheses per round trip, so several k_plane_score launches
  that each write their own rows of the count table and a k_plane_fold_cnt
  over more than 256 rows: scatter_1000 (the winner is iteration 881) and
  wall30 (k drops to 682 inside the batch) at batches 257, 1000, 4096 and
  5000, which is clamped to 4096;
- more than 256 hypotheses that tie on the best count, so k_plane_err in
  several groups with the least rmse carried across them on the host:
  layers_jitter_late (the winner is in the second group), layers_jitter_early
  (the second group must not displace it) and layers_exact (every rmse is 0.0:
  the earliest stays) -- at the default batch and at 4096;
- more than 256 chunks, so k_plane_fold_sum's second pass and
  k_plane_fold_cnt's second stride: wall_1m (1 048 577 points), twice;
- the det_x and det_y branches of the final fit: wall_x, wall_y; lattice_x and
  lattice_y, where the other two determinants are exactly 0.0; wall_diag,
  where the three are within 1 % of each other;
- ransac_n 4 and 16 (rn4, rn16, rn16_n16: 16 points), 2 and 17 refused, and
  k = -inf after pow(fitness, 16) vanishes: rn16_low_fitness_2 and _20;
- the ends of the walk: zero_iterations, and flat (a fitness of exactly 1);
- a distance exactly equal to the threshold: strict_closed, strict_open;
- NaN and infinite coordinates, sampled by hypotheses 0, 1 and 2: nonfinite
  (what the library does today, pinned: such points are never inliers);
- a last chunk without NaN padding: full_chunks_4096, full_chunks_8192.

The inputs come from tests/plane_cases.py; tests/test_plane_oracle.py proves on
the CPU that each one reaches its path.

Not covered, deliberately: a cloud of 2^31 points or more is refused before
any launch, and that refusal is not exercised (48 GiB of coordinates)."""
import numpy as np
import pytest
import torch

from tests import plane_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mg():
    from structured_light_for_3d_model_replication_amd import merge
    return merge


def _run(mg, name, batch=0):
    P, kw = pc.case(name)
    return mg.segment_plane(np.array(P), kw["distance_threshold"], kw["ransac_n"], kw["num_iterations"],
                            kw["probability"], seed=kw["seed"], batch=batch)


def _same(mg, name, batch=0):
    """test_gpu_background._same on a case: everything equals the oracle's."""
    P, _ = pc.case(name)
    model, inl, info = _run(mg, name, batch)
    em, ei, eit = pc.oracle(name)
    print(name, "batch", batch, "iterations", info["iterations"], "oracle", eit, "inliers", len(inl), "oracle",
          len(ei), "model", model, "oracle", em)
    assert info["iterations"] == eit
    np.testing.assert_array_equal(inl.cpu().numpy(), ei)
    np.testing.assert_array_equal(model, em)
    rest = np.setdiff1d(np.arange(len(P)), ei)
    np.testing.assert_array_equal(info["rest"].cpu().numpy(), rest)
    return model, inl, info


@pytest.mark.parametrize("name", pc.CASES)
def test_case_vs_oracle(mg, name):
    _same(mg, name)


@pytest.mark.parametrize("batch", [257, 1000, 4096, 5000])
@pytest.mark.parametrize("name", pc.BATCH_CASES)
def test_batches_above_256_vs_oracle(mg, name, batch):
    """Each equals the oracle, so all equal each other and the default batch:
    test_batch_size_does_not_change_the_result past one scoring launch."""
    _same(mg, name, batch)


@pytest.mark.parametrize("name", pc.TIE_CASES)
def test_more_than_256_ties_in_batches_of_4096(mg, name):
    _same(mg, name, 4096)


def test_ransac_n_limits(mg):
    P, _ = pc.case("rn16")
    for rn in (2, 17):
        with pytest.raises(ValueError):
            mg.segment_plane(np.array(P), 10.0, rn, 100, seed=7)
    with pytest.raises(ValueError):
        mg.segment_plane(np.array(P[:15]), 10.0, 16, 100, seed=7)  # fewer points than ransac_n
    assert len(pc.case("rn16_n16")[0]) == 16
    _same(mg, "rn16_n16")


def test_nonfinite_points_go_to_the_rest(mg):
    model, inl, info = _same(mg, "nonfinite")
    bad = pc.nonfinite_indices()
    assert np.isfinite(model).all()
    assert np.isin(bad, info["rest"].cpu().numpy()).all()
    assert not np.isin(bad, inl.cpu().numpy()).any()


def test_zero_iterations_then_a_run_on_the_same_engine(mg):
    P, _ = pc.case("zero_iterations")
    model, inl, info = _same(mg, "zero_iterations")
    assert np.array_equal(model, np.zeros(4)) and len(inl) == 0 and info["iterations"] == 0
    np.testing.assert_array_equal(info["rest"].cpu().numpy(), np.arange(len(P)))
    _same(mg, "wall_x")


def test_wall_1m_twice(mg):
    a = _run(mg, "wall_1m")
    b = _run(mg, "wall_1m")
    np.testing.assert_array_equal(a[0], b[0])
    assert torch.equal(a[1], b[1]) and torch.equal(a[2]["rest"], b[2]["rest"])
    assert a[2]["iterations"] == b[2]["iterations"]
    np.testing.assert_array_equal(a[1].cpu().numpy(), pc.oracle("wall_1m")[1])
