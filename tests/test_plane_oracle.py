"""tests/plane_oracle.py -- the CPU restatement of the plane RANSAC
(sl_segment_plane, csrc/slplane.inl) -- does what a background removal needs.
Open3D is not installed: parity with Open3D is unpinned, and these tests check
the restatement's own properties (the GPU is checked against it bit for bit in
test_gpu_background.py)."""
import math

import numpy as np
import pytest

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
