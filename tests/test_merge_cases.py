"""Every builder of tests/merge_cases.py meets the condition it was built for,
shown with oracle/merge_oracle.py alone (no GPU): a case of
tests/test_gpu_merge_edges.py cannot quietly stop exercising its branch."""
import numpy as np
import pytest

from oracle import merge_oracle as mo
from tests import merge_cases as mc


# ------------------------------------------------------------------ oracle ----
def test_knn_mean_distances_queries_are_a_subset():
    P = mc.surface_cloud(1300, seed=5)
    rng = np.random.default_rng(6)
    q = rng.permutation(len(P))[:700]  # more than one chunk, unsorted
    for k in (1, 7, 20):
        full = mo.knn_mean_distances(P, k)
        np.testing.assert_array_equal(mo.knn_mean_distances(P, k, queries=q), full[q])
        np.testing.assert_array_equal(mo.knn_mean_distances(P, k, chunk=100, queries=q), full[q])
    assert mo.knn_mean_distances(P, 5, queries=np.zeros(0, np.int64)).shape == (0,)
    few = P[:4]
    np.testing.assert_array_equal(mo.knn_mean_distances(few, 20, queries=[3, 0]), mo.knn_mean_distances(few, 20)[[3, 0]])


# ------------------------------------------------------------------- voxel ----
def test_pass_sweep_covers_every_radix_pass_count():
    passes, wide = set(), 0
    for p in mc.PASS_COUNTS:
        P, C, vs = mc.pass_sweep(p)
        assert P.shape == (4100, 3) and C.shape == (4100, 3)
        assert mc.RS_TILE < len(P) < 2 * mc.RS_TILE
        idx, dims, _ = mc.oracle_grid(P, vs)
        assert tuple(dims) == mc.pass_sweep_dims(p)
        assert mc.radix_passes(dims) == p
        assert mc.key_bits(dims) <= 63
        keys = mc.linear_keys(idx, dims)
        assert 0 <= min(keys) and max(keys) == int(dims[0]) * int(dims[1]) * int(dims[2]) - 1
        wide += max(keys) >= 2 ** 32
        # the oracle's own int64 keys do not wrap
        assert keys == ((idx[:, 0] * dims[1] + idx[:, 1]) * dims[2] + idx[:, 2]).tolist()
        assert np.max(np.unique(keys, return_counts=True)[1]) >= 4  # voxels with several points
        passes.add(mc.radix_passes(dims))
    assert passes == set(range(1, 17))
    assert wide >= 8
    Q, _ = mo.voxel_down_sample(*mc.pass_sweep(16))
    assert 900 < len(Q) <= 1025


def test_voxel_tile_edges_sizes_and_occupancy():
    assert set(mc.VOXEL_TILE_N) == {2, 3, 255, 256, 257, 4095, 4096, 4097, 8192, 8193}
    for n in mc.VOXEL_TILE_N:
        P, C, vs = mc.voxel_tile_edge(n)
        assert len(P) == n == len(C)
        Q, _ = mo.voxel_down_sample(P, C, vs)
        if n == 2:
            assert len(Q) == 1
        elif n == 3:
            assert len(Q) == 2
        else:
            assert 1.5 < n / len(Q) < 8.0


def test_long_voxel_sum_depends_on_order():
    P, C, vs = mc.long_voxel()
    assert len(P) == 10_000 > 2 * mc.RS_TILE
    Q, _ = mo.voxel_down_sample(P, C, vs)
    assert Q.shape == (1, 3)
    decades = np.floor(np.log10(P)).astype(int)
    assert decades.max() - decades.min() >= 8  # eight decades and more
    for seed in range(3):
        perm = np.concatenate([[0, 1], 2 + np.random.default_rng(seed).permutation(len(P) - 2)])
        Q2, _ = mo.voxel_down_sample(P[perm], C[perm], vs)
        assert Q2.shape == (1, 3)
        assert np.all(Q2 != Q)  # on all three axes
    P1, C1, vs1 = mc.one_point_per_voxel()
    assert len(P1) == mc.RS_TILE + 1
    assert len(mo.voxel_down_sample(P1, C1, vs1)[0]) == len(P1)


def test_byte_pairs_defeat_both_rounding_shortcuts():
    P, C, vs, a, b = mc.byte_pairs()
    assert len(P) == 131072 + 65280
    for ch in range(3):  # every pair, once, in every channel
        assert len(np.unique(a[:, ch].astype(int) * 256 + b[:, ch])) == 65536
    assert not np.array_equal(a[:, 0], a[:, 1]) and not np.array_equal(a[:, 1], a[:, 2])
    idx, dims, _ = mc.oracle_grid(P, vs)
    assert tuple(dims) == (256, 256, 2)
    keys = np.array(mc.linear_keys(idx, dims))
    np.testing.assert_array_equal(keys[:65536], 2 * np.arange(65536))
    np.testing.assert_array_equal(keys[65536:131072], 2 * np.arange(65536))
    np.testing.assert_array_equal(keys[131072:], np.repeat(512 * np.arange(256) + 1, 255))
    _, Ce = mo.voxel_down_sample(P, C, vs)
    uk = np.unique(keys)
    assert len(Ce) == len(uk) == 65536 + 256
    pairs = Ce[uk % 2 == 0].astype(int)
    s = a.astype(int) + b.astype(int)
    half_away = (s + 1) // 2
    half_even = np.rint(s / 2.0).astype(int)
    for ch in range(3):
        assert np.any(pairs[:, ch] != half_away[:, ch])
        assert np.any(pairs[:, ch] != half_even[:, ch])
    assert np.all(np.abs(pairs - s / 2.0) <= 0.5)
    equal = Ce[uk % 2 == 1].astype(int)
    assert np.all(np.abs(equal - np.arange(256)[:, None]) <= 1)


def test_faces_and_inexact_quotients():
    P, _, vs = mc.faces("lattice_vs2")
    _, _, lo = mc.oracle_grid(P, vs)
    q = (P - lo) / vs
    assert np.all(q[P % 2 == 1] == np.round(q[P % 2 == 1]))  # exactly on voxel faces
    assert np.all(q[P == P.max()] == 4.0)                     # the maximum point included
    P, _, vs = mc.faces("tenths")
    _, _, lo = mc.oracle_grid(P, vs)
    assert np.sum(np.floor((P - lo) / vs) != np.floor((P - lo) * (1.0 / vs))) > 100
    P, _, vs = mc.faces("tenths_negative")
    _, _, lo = mc.oracle_grid(P, vs)
    q = (P - lo) / vs
    assert np.any((q != np.round(q)) & (np.abs(q - np.round(q)) < 1e-9))  # an ulp or so off an integer
    assert mc.faces("tenths_negative")[0].min() < -10.0
    P, _, vs = mc.faces("offset_1e7")
    assert np.abs(P).min() > 9.9e6 and P[:, 1].max() < 0
    assert 300 < len(mo.voxel_down_sample(P, None, vs)[0]) < len(P)


def test_limit_clouds_sit_either_side_of_the_axis_limit():
    for e, voxels in ((mc.GRID_MAX_E, 2_000_001), (mc.GRID_MAX_E + 1, 2_000_002)):
        P, C, vs = mc.limit_cloud(e)
        _, dims, lo = mc.oracle_grid(P, vs)
        assert tuple(dims) == (voxels, 1, 1)
        # not Open3D's "voxel_size is too small" rejection
        assert vs * float(2 ** 31 - 1) >= ((P.max(0) + vs * 0.5) - lo).max()
        assert len(mo.voxel_down_sample(P, C, vs)[0]) == 2


# ---------------------------------------------------- statistical outliers ----
def test_k_sweep_values():
    assert mc.K_SWEEP == (2, 3, 19, 21, 31)
    assert set(mc.SMALL_N) == {(20, 1), (20, 2), (20, 19), (20, 20), (20, 21), (7, 1), (7, 2), (7, 6), (7, 7), (7, 8)}


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_sor_tile_edges_keep_and_reject_everywhere(n):
    P = mc.sor_tile_edge(n)
    assert len(P) == n
    ind, _ = mo.remove_statistical_outlier(P, 20, 2.0)
    keep = np.zeros(n, bool)
    keep[ind] = True
    for a in range(0, n - 1, mc.KT):  # every run of 256 (and so every scan tile of 4096)
        assert keep[a:a + mc.KT].any() and not keep[a:a + mc.KT].all()
    if n == mc.RS_TILE + 1:
        assert not keep[mc.RS_TILE] and keep[mc.RS_TILE - 1]  # the last tile holds one rejected point


def test_blob_scene_isolated_query_looks_into_the_corner_blob():
    P, b_idx, iso_idx = mc.blob_scene()
    assert 2000 < len(P) < 5000 and len(iso_idx) == 10
    np.testing.assert_array_equal(P.max(0), mc.BLOB_B_CORNER)
    assert np.all(P[b_idx[-1]] == P.max(0))  # one point of blob B is the maximum corner itself
    q = P[iso_idx[0]]
    d = ((q - P) ** 2).sum(1)
    nearest = np.argsort(d, kind="stable")[1:33]  # itself first
    assert np.all(np.isin(nearest, b_idx))
    # isolated: every such point's nearest other point is far beyond the blobs' size
    for i in iso_idx:
        dd = ((P[i] - P) ** 2).sum(1)
        dd[i] = np.inf
        assert dd.min() > 30.0 ** 2


def test_shell_scene_is_an_exact_shell_around_its_centre():
    P, q = mc.shell_scene()
    n = mc.SHELL_N
    assert len(P) == n + 4 and np.all(P[n] == 0.0)
    r = np.sqrt((P[:n] ** 2).sum(1))
    assert np.all(np.abs(r - 300.0) < 1e-9)
    assert len(q) == 4 + 512 == len(np.unique(q)) and q[0] == n
    assert np.all(np.sqrt((P[n + 1:] ** 2).sum(1)) > 700.0)


def test_degenerate_clouds_are_degenerate():
    ext = lambda P: P.max(0) - P.min(0)  # noqa: E731
    assert ext(mc.degenerate("plane"))[2] == 0.0 and np.all(ext(mc.degenerate("plane"))[:2] > 40.0)
    e = ext(mc.degenerate("line_x"))
    assert e[0] > 90.0 and e[1] == 0.0 and e[2] == 0.0
    P = mc.degenerate("line_diagonal")
    assert np.all(P[:, 0] == P[:, 1]) and np.all(P[:, 1] == P[:, 2]) and ext(P)[0] > 90.0
    P = mc.degenerate("coincident_but_one")
    assert len(P) == 40 and len(np.unique(P, axis=0)) == 2 and np.all(P[:39] == P[0])
    P = mc.degenerate("lattice9")
    assert len(P) == 729
    for k in (5, 20):  # exact ties across the k-th neighbour
        d = np.sort(((P[364] - P) ** 2).sum(1))
        assert d[k - 1] == d[k]
    P = mc.degenerate("blobs_far")
    assert P.min() > 0.99 * mc.FAR_OFFSET and len(np.unique(P, axis=0)) > len(P) - 10
    d = np.sqrt(((P[:200, None] - P[None, :mc.BLOB_N]) ** 2).sum(2))
    d[d == 0] = np.inf
    assert 1e-6 < np.median(d.min(1)) < 1e-3  # spacings far above an ulp of 1e9 (1.2e-7)
    # the search margin, 1e-12 * (sum of |coordinate|), is above 2.5 % of the scene's extent: wider
    # than cells sized for 5 to 20 of 3 010 points (the GPU test shows it from the library's counts)
    assert 1e-12 * np.abs(P).sum(1).min() > 0.025 * ext(P).max()


def test_collinear_cloud_is_collinear():
    P = mc.collinear()
    e = P.max(0) - P.min(0)
    assert len(P) == 4000 and e[0] > 990.0 and e[1] == 0.0 and e[2] == 0.0
