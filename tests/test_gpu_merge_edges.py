"""The merge primitives of csrc/slmerge.hip (bounds, 64-bit radix sort, tile
scans, segment heads, cell pyramid, the three kNN kernels) at the sizes, key
widths and degenerate inputs that tests/test_gpu_merge.py never reaches, bit
for bit against oracle/merge_oracle.py.  The inputs are tests/merge_cases.py's;
tests/test_merge_cases.py shows on the CPU that each reaches its branch.  The
mutation table of DESIGN.md C.1 records which kernel faults each test catches."""
import functools
import re

import numpy as np
import pytest

from oracle import merge_oracle as mo
from tests import merge_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mg():
    from structured_light_for_3d_model_replication_amd import merge
    return merge


def _check_voxel(mg, P, C, vs):
    """GPU == oracle: points and colours, and the points again without colours."""
    Qe, Ce = mo.voxel_down_sample(P, C, vs)
    Q, Cq = mg.voxel_down_sample(P, C, vs)
    np.testing.assert_array_equal(Q.cpu().numpy(), Qe)
    np.testing.assert_array_equal(Cq.cpu().numpy(), Ce)
    Q2, C2 = mg.voxel_down_sample(P, None, vs)
    assert C2 is None
    np.testing.assert_array_equal(Q2.cpu().numpy(), Qe)
    return Qe, Ce


@functools.lru_cache(maxsize=None)
def _sor_expected(builder, arg, k):
    """The oracle's (ind, avg) of a named cloud, computed once per (cloud, k)."""
    return mo.remove_statistical_outlier(_sor_cloud(builder, arg), k, 2.0)


def _sor_cloud(builder, arg):
    if builder == "surface":
        return mc.surface_cloud(1500, seed=31)[:arg]
    if builder == "tile":
        return mc.sor_tile_edge(arg)
    if builder == "blobs":
        return mc.blob_scene()[0]
    if builder == "collinear":
        return mc.collinear()
    return mc.degenerate(arg)


def _check_sor(mg, builder, arg, k):
    P = _sor_cloud(builder, arg)
    ind_e, avg_e = _sor_expected(builder, arg, k)
    ind, avg = mg.remove_statistical_outlier(P, k, 2.0)
    np.testing.assert_array_equal(avg.cpu().numpy(), avg_e)
    np.testing.assert_array_equal(ind.cpu().numpy(), ind_e)


def _stats(err):
    """The numbers of the library's SLGPU_MERGE_STATS lines (the slow / overflow
    line is printed only when some query left the fast kernel)."""
    out = {"slow": 0, "overflow": 0}
    m = re.search(r"\[slmerge\] slow=(\d+) overflow=(\d+)", err)
    if m:
        out["slow"], out["overflow"] = int(m.group(1)), int(m.group(2))
    m = re.search(r"\[slmerge\] n=(\d+) .*\bl0=(\d+) levels=(\d+) sort_bits=(\d+)", err)
    assert m, err
    out["n"], out["l0"], out["levels"], out["sort_bits"] = (int(g) for g in m.groups())
    return out


# ------------------------------------------------------------------- voxel ----
@pytest.mark.parametrize("passes", mc.PASS_COUNTS)
def test_voxel_every_radix_pass_count(mg, passes):
    """Key widths of 3 .. 63 bits: 1 .. 16 radix passes (odd counts end in the
    scratch pair and are copied back), digits above bit 32 from 9 passes on."""
    _check_voxel(mg, *mc.pass_sweep(passes))


@pytest.mark.parametrize("n", mc.VOXEL_TILE_N)
def test_voxel_tile_edges(mg, n):
    """n at, one below and one above the workgroup (256) and the sort / scan
    tile (4096, 8192); 2 and 3 points."""
    _check_voxel(mg, *mc.voxel_tile_edge(n))


def test_voxel_one_long_voxel(mg):
    """10 000 points of one voxel, three sort tiles: the sums are the oracle's
    only if the sort keeps the points in index order (stability within a
    thread, across threads and across tiles)."""
    Qe, _ = _check_voxel(mg, *mc.long_voxel())
    assert Qe.shape == (1, 3)


def test_voxel_one_point_per_voxel(mg):
    Qe, _ = _check_voxel(mg, *mc.one_point_per_voxel())
    assert len(Qe) == mc.RS_TILE + 1


def test_voxel_every_byte_pair(mg):
    """round(clamp(sum(c / 255) / m) * 255) on every byte pair in every channel,
    and on 255 equal bytes."""
    P, C, vs, _, _ = mc.byte_pairs()
    _check_voxel(mg, P, C, vs)


@pytest.mark.parametrize("name", mc.FACE_CASES)
def test_voxel_faces_and_inexact_quotients(mg, name):
    _check_voxel(mg, *mc.faces(name))


def test_voxel_axis_limit(mg):
    """2 000 001 voxels on an axis are accepted, 2 000 002 are rejected (by the
    grid check, not by "voxel_size is too small"), and the engine works after."""
    P, C, vs = mc.limit_cloud(mc.GRID_MAX_E)
    _check_voxel(mg, P, C, vs)
    P2, C2, vs2 = mc.limit_cloud(mc.GRID_MAX_E + 1)
    with pytest.raises(ValueError, match="voxel grid exceeds"):
        mg.voxel_down_sample(P2, C2, vs2)
    _check_voxel(mg, P, C, vs)
    _check_voxel(mg, *mc.voxel_tile_edge(mc.RS_TILE + 1))


# ---------------------------------------------------- statistical outliers ----
@pytest.mark.parametrize("k", mc.K_SWEEP)
def test_sor_k_sweep(mg, k):
    """The kMaxK register list with the k-th entry picked by the select."""
    _check_sor(mg, "surface", 1500, k)


@pytest.mark.parametrize("k,n", mc.SMALL_N)
def test_sor_fewer_points_than_neighbours(mg, k, n):
    _check_sor(mg, "surface", n, k)


@pytest.mark.parametrize("n", [mc.RS_TILE - 1, mc.RS_TILE, mc.RS_TILE + 1])
def test_sor_tile_edges(mg, n):
    _check_sor(mg, "tile", n, 20)


@pytest.mark.parametrize("k", [7, 20, 32])
def test_sor_isolated_queries_all_three_kernels(mg, k, monkeypatch, capfd):
    """Two blobs and ten isolated points, one blob in the Morton-last cell of
    every level: the fast kernel, the best-first search and (SLGPU_MERGE_CLIMB)
    the pyramid climb all equal the oracle on every point."""
    monkeypatch.setenv("SLGPU_MERGE_STATS", "1")
    capfd.readouterr()
    _check_sor(mg, "blobs", None, k)
    best = _stats(capfd.readouterr().err)
    assert best["slow"] > 0
    monkeypatch.setenv("SLGPU_MERGE_CLIMB", "1")
    _check_sor(mg, "blobs", None, k)
    climb = _stats(capfd.readouterr().err)
    assert climb["slow"] > 0


def test_sor_frontier_overflow(mg, monkeypatch, capfd):
    """A query at the centre of an exact sphere shell with k = 2: its frontier
    outgrows kBestCap and the query goes on to the pyramid climb."""
    P, q = mc.shell_scene()
    monkeypatch.setenv("SLGPU_MERGE_STATS", "1")
    capfd.readouterr()
    ind, avg = mg.remove_statistical_outlier(P, mc.SHELL_K, 2.0)
    st = _stats(capfd.readouterr().err)
    assert st["slow"] > 0 and st["overflow"] > 0
    a = avg.cpu().numpy()
    np.testing.assert_array_equal(a[q], mo.knn_mean_distances(P, mc.SHELL_K, queries=q))
    np.testing.assert_array_equal(ind.cpu().numpy(), mo.statistical_outlier_indices(a, 2.0))
    monkeypatch.setenv("SLGPU_MERGE_CLIMB", "1")
    ind_c, avg_c = mg.remove_statistical_outlier(P, mc.SHELL_K, 2.0)
    np.testing.assert_array_equal(a, avg_c.cpu().numpy())
    np.testing.assert_array_equal(ind.cpu().numpy(), ind_c.cpu().numpy())


@pytest.mark.parametrize("k", [20, 5])
@pytest.mark.parametrize("name", mc.DEGENERATE_CASES)
def test_sor_degenerate_extents(mg, name, k, monkeypatch, capfd):
    monkeypatch.setenv("SLGPU_MERGE_STATS", "1")
    capfd.readouterr()
    _check_sor(mg, "degenerate", name, k)
    st = _stats(capfd.readouterr().err)
    if name == "blobs_far":
        # 1e9 from the origin the search margin is wider than the cells: no
        # query settles in the fast kernel, and every mean is still exact
        assert st["slow"] == st["n"] == len(mc.degenerate(name))


@pytest.mark.parametrize("k", [1, 2])
def test_sor_wide_morton_keys(mg, k, monkeypatch, capfd):
    """A collinear cloud: the volume floor gives a fine cell, 14 bits per axis,
    and the Morton sort runs past bit 32."""
    monkeypatch.setenv("SLGPU_MERGE_STATS", "1")
    capfd.readouterr()
    _check_sor(mg, "collinear", None, k)
    st = _stats(capfd.readouterr().err)
    assert st["levels"] >= 12
    assert st["sort_bits"] >= 36  # 12 or more bits per axis: the x axis' bit 11 is key bit 33
