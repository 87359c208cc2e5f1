"""The merge stage (csrc/slmerge.hip and the .inl files it includes) on poisoned scratch and on a side stream.

Every other GPU suite runs its entry points on whatever the scratch pool happens to hold (often fresh, zero pages)
and on the legacy null stream, with which every blocking stream synchronises.  Here every entry point that takes
scratch from the pool runs with each buffer filled beforehand (merge.pool_poison, sl_merge_pool_poison):

- 0xFF on the current stream: a double reads as NaN, an integer as -1 / the maximum;
- 0x55 on the current stream: a double reads as 1.19e103, an integer as 0x55555555;
- 0xFF inside ``with torch.cuda.stream(side)``, upload and download included, ``side`` a fresh non-blocking stream;
- 0xFF, the row's largest case and at once its smallest, both poisoned: a small request after large ones is served
  from what the pool holds by then (a kept buffer of at most twice its size, else a fresh one), the order in which a
  360 merge on growing and shrinking clouds meets the pool.

The inputs, oracles and assertions are the features' own (tests/*_cases.py and the helpers of their GPU suites): bit
for bit.  Each call must also have drawn scratch from the pool (the poison counter grows), so a row cannot pass by
not being exercised.  Then the pool itself: trim, the call after a trim, the switch's arguments.

Oracle results are computed once per process and shared with the features' own suites (their ``solved`` / ``oracle``
/ ``lru_cache`` helpers, or an ``lru_cache`` here); the one slow oracle, bpa_oracle's dense_blob (seconds), is the
one tests/test_gpu_bpa.py has already computed when the whole suite runs.  On the MI355X: 131 items, 14 s, no
mismatch; DESIGN.md C.1 lists the bytes poisoned per row."""
import functools
import time

import numpy as np
import pytest
import torch

from oracle import merge_oracle as mo
from oracle import registration_oracle as ro
from tests import bpa_oracle as bo
from tests import cluster_cases as cc
from tests import cluster_oracle as co
from tests import merge_cases as mc
from tests import mesh_cases as pmc
from tests import mesh_oracle as pmo
from tests import meshclean_cases as cs
from tests import meshclean_oracle as oc
from tests import meshwrite_oracle as wo
from tests import orient_oracle as oo
from tests import posegraph_cases as pgc
from tests import registration_cases as rc
from tests import test_gpu_background as t_background
from tests import test_gpu_bpa as t_bpa
from tests import test_gpu_cluster_paths as t_cluster
from tests import test_gpu_merge as t_merge
from tests import test_gpu_merge_edges as t_edges
from tests import test_gpu_mesh_paths as t_poisson
from tests import test_gpu_meshclean as t_clean
from tests import test_gpu_meshwrite as t_write
from tests import test_gpu_orient as t_orient
from tests import test_gpu_plane_paths as t_plane
from tests import test_gpu_registration_paths as t_reg

pytestmark = pytest.mark.gpu

# (id, poison byte, on a side stream)
CONDITIONS = (("ff", 0xFF, False), ("55", 0x55, False), ("ff_side_stream", 0xFF, True))

# The wrappers the matrix has to hold at the least -> their rows ("splat", "divergence" and "sample" are kernels
# without scratch of their own: mesh.poisson_field runs them, and its iso value takes the pool's ordered sum).
_CHAIN = "poisson_field[splat,divergence,sample,ordered_sum]"
REQUIRED = {
    "voxel_down_sample": ["voxel_down_sample"], "remove_statistical_outlier": ["remove_statistical_outlier"],
    "estimate_normals": ["estimate_normals"], "radius_search": ["radius_search"],
    "compute_fpfh_feature": ["compute_fpfh_feature"], "feature_nn": ["feature_nn"],
    "registration_ransac_based_on_feature_matching": ["registration_ransac_based_on_feature_matching"],
    "registration_icp": ["registration_icp"],
    "get_information_matrix_from_point_clouds": ["get_information_matrix_from_point_clouds"],
    "segment_plane": ["segment_plane"], "cluster_dbscan": ["cluster_dbscan"],
    "remove_radius_outlier": ["remove_radius_outlier"],
    "compute_nearest_neighbor_distance": ["compute_nearest_neighbor_distance"],
    "orient_normals_mst": ["orient_normals_mst"], "ball_pivot_candidates": ["ball_pivot_candidates"],
    "create_from_point_cloud_ball_pivoting": ["create_from_point_cloud_ball_pivoting"],
    "splat": [_CHAIN], "divergence": [_CHAIN], "sample": [_CHAIN],
    "extract": ["extract_isosurface"], "trim_by_density": ["trim_by_density"],
    "cluster_connected_triangles": ["cluster_connected_triangles[areas]", "cluster_connected_triangles[no areas]"],
    "remove_triangles_by_mask": ["remove_triangles_by_mask"],
    "remove_unreferenced_vertices": ["remove_unreferenced_vertices"],
    "simplify_vertex_clustering": ["simplify_vertex_clustering"],
    "compute_triangle_normals": ["compute_triangle_normals"], "compute_vertex_normals": ["compute_vertex_normals"],
    "write_triangle_mesh": ["write_triangle_mesh[.stl]", "write_triangle_mesh[.ply]"],
}


def _cube_cloud():
    rng = np.random.default_rng(3)
    return rng.normal(size=(1000, 3)), rng.integers(0, 256, (1000, 3), dtype=np.uint8)


# Wrappers of the merge stage whose call path takes no scratch from the pool: not rows of the matrix, and
# test_no_scratch_wrappers_take_none holds each to it -> (wrapper, why, a call of it).
NO_SCRATCH = (
    ("select_by_index[not inverted]", "one gather kernel from the inputs to the outputs",
     lambda mg, ms: mg.select_by_index(*_cube_cloud(), np.arange(0, 1000, 3))),
    ("transform", "one kernel, in place on a copy", lambda mg, ms: mg.transform(_cube_cloud()[0], np.eye(4))),
    ("orient_normals_towards_camera_location", "one kernel, in place on a copy",
     lambda mg, ms: ms.orient_normals_towards_camera_location(*pmc.orient_case(257)[:3])),
    ("solve", "torch's FFT: torch's allocator, not the pool",
     lambda mg, ms: ms.solve(t_poisson._dev(ms, pmc.solve_case(3, 0, 0.0)), pmc.SOLVE_H)),
)


@pytest.fixture(scope="module")
def mg():
    from structured_light_for_3d_model_replication_amd import merge
    return merge


@pytest.fixture(scope="module")
def ms():
    from structured_light_for_3d_model_replication_amd import mesh
    return mesh


@pytest.fixture(scope="module", autouse=True)
def disarmed_afterwards():
    """Whatever happens in this module, the modules after it run on an unpoisoned pool."""
    from structured_light_for_3d_model_replication_amd import _lib
    t0 = time.perf_counter()
    try:
        yield
    finally:
        assert _lib.load().sl_merge_pool_poison(-1, None) == _lib.SL_OK
        print(f"\ntests/test_gpu_dirty_scratch.py: {time.perf_counter() - t0:.1f} s")


# ---- the rows: name -> checks, the smallest non-empty case first, the largest last ---------------------------
# A check is a callable of (mg, ms, tmp_path) that runs the wrapper and makes its feature's own assertion.
ROWS = {}


def row(name, *checks):
    ROWS[name] = checks


# -- merge -----------------------------------------------------------------------------------------------------
row("voxel_down_sample",
    lambda mg, ms, d: t_edges._check_voxel(mg, *mc.voxel_tile_edge(3)),
    lambda mg, ms, d: t_edges._check_voxel(mg, *mc.voxel_tile_edge(mc.RS_TILE + 1)))

row("remove_statistical_outlier",
    lambda mg, ms, d: t_edges._check_sor(mg, "surface", 21, 20),
    lambda mg, ms, d: t_edges._check_sor(mg, "tile", mc.RS_TILE + 1, 20))


@functools.lru_cache(maxsize=None)
def _normals_case(name):
    """test_gpu_merge.test_estimate_normals_vs_oracle's lattice_ties and max_nn_32 -> (P, radius, max_nn, oracle)."""
    P, radius, max_nn = {"lattice_ties": (t_merge._lattice(9), 2.01, 30),
                         "max_nn_32": (t_merge._cloud(2000, seed=6, scale=40.0)[0], 8.0, 32)}[name]
    return P, radius, max_nn, mo.estimate_normals(P, radius, max_nn)


def _normals(mg, name):
    P, radius, max_nn, want = _normals_case(name)
    np.testing.assert_array_equal(mg.estimate_normals(P, radius, max_nn).cpu().numpy(), want)


row("estimate_normals",
    lambda mg, ms, d: _normals(mg, "lattice_ties"),
    lambda mg, ms, d: _normals(mg, "max_nn_32"))

row("radius_search",
    lambda mg, ms, d: t_reg._radius_equal(mg, "n65", 100),
    lambda mg, ms, d: t_reg._radius_equal(mg, "c1024", 1024),
    lambda mg, ms, d: t_reg._radius_equal(mg, "c1025", 100))

_FPFH_SMALL = (np.array([[0.0, 0, 0], [100.0, 0, 0], [100.5, 0, 0], [100.0, 0.5, 0.2]]),
               np.array([[0.0, 0, 1], [0, 0, 1], [0, 1, 0], [1, 0, 0]]), 2.0, 100)


@functools.lru_cache(maxsize=None)
def _fpfh_case(name):
    """test_gpu_registration.test_fpfh_vs_oracle's four points; test_fpfh_degenerate_cloud_vs_oracle at max_nn 16."""
    P, N, radius, max_nn = _FPFH_SMALL if name == "four" else (*rc.fpfh_cloud(), rc.FPFH_RADIUS, 16)
    return P, N, radius, max_nn, ro.compute_fpfh(P, N, radius, max_nn)


def _fpfh(mg, name):
    P, N, radius, max_nn, want = _fpfh_case(name)
    np.testing.assert_array_equal(mg.compute_fpfh_feature(P, N, radius, max_nn).cpu().numpy(), want)


row("compute_fpfh_feature",
    lambda mg, ms, d: _fpfh(mg, "four"),
    lambda mg, ms, d: _fpfh(mg, "degenerate"))

row("feature_nn",
    lambda mg, ms, d: t_reg.test_feature_nn_shapes_vs_oracle(mg, 1, 65),
    lambda mg, ms, d: t_reg.test_feature_nn_shapes_vs_oracle(mg, 257, 65),
    lambda mg, ms, d: t_reg.test_feature_nn_shapes_vs_oracle(mg, 700, 64 * 15 + 1))

row("registration_ransac_based_on_feature_matching",
    lambda mg, ms, d: t_reg.test_ransac_paths_vs_oracle(mg, "r4"),
    lambda mg, ms, d: t_reg.test_ransac_paths_vs_oracle(mg, f"r3_{rc.BATCH + 1}"))

row("registration_icp",
    lambda mg, ms, d: t_reg.test_icp_equidistant_targets_tie_to_the_lower_index(mg, None),
    lambda mg, ms, d: t_reg.test_icp_equidistant_targets_tie_to_the_lower_index(mg, 2e4))


def _information(mg, name):
    S, T, dist, M = pgc.info_case(name)
    want, want_n = pgc.info_oracle(name)
    got, got_n = mg.get_information_matrix_from_point_clouds(S, T, dist, M, info=True)
    np.testing.assert_array_equal(got, want)
    assert got_n == want_n


row("get_information_matrix_from_point_clouds",
    lambda mg, ms, d: _information(mg, "blob1_moved"),
    lambda mg, ms, d: _information(mg, "gap"),
    lambda mg, ms, d: _information(mg, "blob129_moved"))

row("segment_plane",
    lambda mg, ms, d: t_plane._same(mg, "rn16_n16"),
    lambda mg, ms, d: t_plane._same(mg, "wall30", 257))

@functools.lru_cache(maxsize=None)
def _invert_case(m):
    """voxel_tile_edge(4097)'s cloud and m listed indices (every third, shuffled) -> (P, C, ind, the rest)."""
    P, C, _ = mc.voxel_tile_edge(mc.RS_TILE + 1)
    ind = np.random.default_rng(m).permutation(np.arange(0, len(P), 3)[:m])
    return P, C, ind, np.setdiff1d(np.arange(len(P)), ind)


def _invert(mg, m):
    """test_gpu_background.test_select_by_index_invert's assertion around the scan's tile (4097 points)."""
    P, C, ind, keep = _invert_case(m)
    Q, Cq = mg.select_by_index(P, C, ind, invert=True)
    np.testing.assert_array_equal(Q.cpu().numpy(), P[keep])
    np.testing.assert_array_equal(Cq.cpu().numpy(), C[keep])


row("select_by_index[invert]",
    lambda mg, ms, d: t_background.test_select_by_index_invert(mg),
    lambda mg, ms, d: _invert(mg, 0),
    lambda mg, ms, d: _invert(mg, 1366))

# -- clustering ------------------------------------------------------------------------------------------------
row("cluster_dbscan",
    lambda mg, ms, d: t_cluster._dbscan(mg, cc.solved("wave_edge_65")),
    lambda mg, ms, d: t_cluster._dbscan(mg, cc.solved("tile_edge_513")))

row("radius_count",
    lambda mg, ms, d: t_cluster._counts(mg, cc.solved("wave_edge_65")),
    lambda mg, ms, d: t_cluster._counts(mg, cc.solved("tile_edge_513")))

row("remove_radius_outlier",
    lambda mg, ms, d: t_cluster.test_remove_radius_outlier(mg, "dust_then_clump"),
    lambda mg, ms, d: t_cluster.test_remove_radius_outlier(mg, "tile_edge_257"))


@functools.lru_cache(maxsize=None)
def _nn_case(name):
    P = t_cluster.NN_CLOUDS[name] if name in t_cluster.NN_CLOUDS else np.array(cc.solved(name)["P"])
    return P, co.nearest_neighbor_distance(P)


def _nn_distance(mg, name):
    P, want = _nn_case(name)
    np.testing.assert_array_equal(t_cluster._twice(lambda: mg.compute_nearest_neighbor_distance(P)), want)


row("compute_nearest_neighbor_distance",
    lambda mg, ms, d: _nn_distance(mg, "three_with_a_duplicate"),
    lambda mg, ms, d: _nn_distance(mg, "wave_edge_64"),
    lambda mg, ms, d: _nn_distance(mg, "tile_edge_513"))

# -- meshing ---------------------------------------------------------------------------------------------------
_ORIENT_ORACLE = {}


def _orient_inputs(name):
    if name == "torus":  # test_gpu_orient.test_torus at (2000, 0.3, k = 12)
        P, out = oo.torus(2000, 2012)
        return P, out * t_orient._signs(2000, 12), 0.3, 12
    g = np.stack(np.meshgrid(np.arange(30.0), np.arange(30.0), indexing="ij"), -1).reshape(-1, 2)
    N = np.zeros((900, 3))  # test_gpu_orient.test_all_ties_lattice
    N[:, 2] = t_orient._signs(900, 5)[:, 0]
    return np.concatenate([g, np.full((900, 1), 0.25)], 1), N, 1.5, 9


def _orient(mg, ms, name):
    """test_gpu_orient._same with the oracle's run kept: the graph must be the one it was computed on."""
    P, N, radius, k = _orient_inputs(name)
    idx, _, cnt = mg.radius_search(P, radius, k)
    idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
    if name not in _ORIENT_ORACLE:
        _ORIENT_ORACLE[name] = (idx, cnt, *oo.orient(P, N, idx, cnt))
    widx, wcnt, exp, tree, comps = _ORIENT_ORACLE[name]
    np.testing.assert_array_equal(cnt, wcnt)
    listed = np.arange(k)[None, :] < cnt[:, None]  # a row's slots past its count are not written
    np.testing.assert_array_equal(idx[listed], widx[listed])
    got, info = ms.orient_normals_mst(P, N, idx, cnt)
    got2, info2 = ms.orient_normals_consistent_tangent_plane(P, N, k, radius=radius, info=True)
    assert info["components"] == comps == info2["components"]
    np.testing.assert_array_equal(info["tree_slots"].cpu().numpy(), tree)
    np.testing.assert_array_equal(got.cpu().numpy(), exp)
    np.testing.assert_array_equal(got2.cpu().numpy(), exp)
    assert torch.equal(info2["tree_slots"], info["tree_slots"])


row("orient_normals_mst",
    lambda mg, ms, d: _orient(mg, ms, "lattice"),
    lambda mg, ms, d: _orient(mg, ms, "torus"))


@functools.lru_cache(maxsize=None)
def _hole_fill_classes():
    """test_gpu_bpa.test_candidates_with_vertex_classes on hole_fill -> (radius, classes, the oracle's candidates)."""
    s = bo.solved("hole_fill")
    n_first = sum(s["info"]["triangles"][:s["info"]["passes"][0]])
    cls = bo.vertex_classes(s["T"][:n_first], len(s["P"]))
    return s["radii"][1], cls, bo.candidates(s["P"], s["N"], s["radii"][1], cls)


def _bpa_classes(ms):
    s = bo.solved("hole_fill")
    r, cls, want = _hole_fill_classes()
    assert {1, 2} <= set(cls.tolist()) and len(want) > 0
    np.testing.assert_array_equal(t_bpa._twice(lambda: ms.ball_pivot_candidates(s["P"], s["N"], r, cls)), want)


def _bpa_candidates(ms, name):
    s = bo.solved(name)
    for r, want in zip(s["radii"], s["candidates"]):
        np.testing.assert_array_equal(t_bpa._twice(lambda: ms.ball_pivot_candidates(s["P"], s["N"], r)), want)


def _bpa_257(ms):
    """test_gpu_bpa.test_neighbourhood_sizes_at_the_kernels_thresholds at 257: two points on the second tier."""
    Q = np.concatenate([bo._TRI, np.tile([[0.4, 0.3, -1.9]], (257 - 3, 1))])
    NQ = np.concatenate([bo._up(3), np.zeros((257 - 3, 3))])
    np.testing.assert_array_equal(t_bpa._twice(lambda: ms.ball_pivot_candidates(Q, NQ, 1.0)), [[0, 1, 2]])
    d = Q[:, None, :] - Q[None, :, :]
    sees = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2] < 4.0).sum(1)
    assert ms.ball_pivot_stats()["second_tier"] == (sees > 256).sum() == 2


row("ball_pivot_candidates",
    lambda mg, ms, d: _bpa_candidates(ms, "patch"),
    lambda mg, ms, d: _bpa_257(ms),
    lambda mg, ms, d: _bpa_classes(ms),
    lambda mg, ms, d: _bpa_candidates(ms, "dense_blob"))


def _bpa_mesh(ms, name):
    s = bo.solved(name)
    V, T, info = ms.create_from_point_cloud_ball_pivoting(s["P"], s["N"], s["radii"], info=True)
    np.testing.assert_array_equal(V.cpu().numpy(), s["P"])
    assert info == s["info"]
    np.testing.assert_array_equal(T.cpu().numpy(), s["T"])


row("create_from_point_cloud_ball_pivoting",
    lambda mg, ms, d: _bpa_mesh(ms, "patch"),
    lambda mg, ms, d: _bpa_mesh(ms, "hole_fill"),
    lambda mg, ms, d: _bpa_mesh(ms, "dense_blob"))


@functools.lru_cache(maxsize=None)
def _splat_oracle(kind, n, depth):
    """tests/mesh_oracle.py on a mesh_cases cloud -> (P, N, scale, origin, h, W, V, div)."""
    P, N, scale = pmc.cloud(kind, n, 1 << depth, seed=n + depth)
    o, h, _ = pmo.box(P, depth, scale)
    W, V = pmo.splat(P, N, o, h, 1 << depth)
    return P, N, scale, o, h, W, V, pmo.divergence(V, h)


def _poisson_field(ms, kind, n, depth):
    """test_gpu_mesh_paths.test_small_grid_chain: splat, un-fix, divergence, the iso value (sample and the ordered
    sum) and the density samples, each on the GPU's own output of the stage before it."""
    P, N, scale, o, h, W, V, div = _splat_oracle(kind, n, depth)
    f = ms.poisson_field(P, N, depth, scale, keep=True)
    t_poisson._same_bits(f["W"].cpu().numpy(), W)
    t_poisson._same_bits(f["V"].cpu().numpy(), V)
    t_poisson._same_bits(f["div"].cpu().numpy(), div)
    chi = f["chi"].cpu().numpy()
    assert f["iso"] == pmo.iso_value(chi, P, o, h)
    Vg, Tg = ms.extract_isosurface(f["chi"], f["iso"], f["origin"], f["h"])
    Vo, To = pmo.extract(chi, f["iso"], o, h)
    np.testing.assert_array_equal(Tg.cpu().numpy(), To)
    t_poisson._same_bits(Vg.cpu().numpy(), Vo)
    if len(Vo):
        t_poisson._same_bits(ms.vertex_density(f["W"], Vg, f["origin"], f["h"]).cpu().numpy(), pmo.sample(W, Vo, o, h))


row("poisson_field[splat,divergence,sample,ordered_sum]",
    lambda mg, ms, d: _poisson_field(ms, "nodes", 257, 2),
    lambda mg, ms, d: _poisson_field(ms, "faces", 4097, 4))


row("ordered_sum",
    lambda mg, ms, d: t_poisson.test_ordered_sum(ms, 257),
    lambda mg, ms, d: t_poisson.test_ordered_sum(ms, 4097),
    lambda mg, ms, d: t_poisson.test_ordered_sum(ms, 4096 * 256 + 1))


@functools.lru_cache(maxsize=None)
def _extract_oracle(name):
    chi, iso = pmc.fields()[name]
    return chi, iso, pmo.extract(chi, iso, pmc.SEAM_ORIGIN, pmc.SEAM_H)


def _extract(ms, name):
    """test_gpu_mesh_paths.test_extraction_fields."""
    chi, iso, (Vo, To) = _extract_oracle(name)
    V, T = ms.extract_isosurface(t_poisson._dev(ms, chi), iso, pmc.SEAM_ORIGIN, pmc.SEAM_H)
    assert len(To) > 0
    np.testing.assert_array_equal(T.cpu().numpy(), To)
    t_poisson._same_bits(V.cpu().numpy(), Vo)


row("extract_isosurface",
    lambda mg, ms, d: _extract(ms, "random4"),
    lambda mg, ms, d: _extract(ms, "random"))


@functools.lru_cache(maxsize=None)
def _trim_case(n):
    """mesh_cases.trim_case's mesh with whole-number densities (the quantile's interpolation is then exact)."""
    V, T, _ = pmc.trim_case(n, n, "none")
    dens = np.random.default_rng(n).integers(0, 1000, len(V)).astype(np.float64)
    return V, T, dens, pmo.remove_vertices_by_mask(V, T, dens < np.quantile(dens, 0.25))


def _trim(ms, n):
    """test_gpu_mesh.test_density_and_trim_bits' assertion."""
    V, T, dens, (Vo, To) = _trim_case(n)
    V2, T2 = ms.trim_by_density(t_poisson._dev(ms, V), t_poisson._dev(ms, T), t_poisson._dev(ms, dens), 0.25)
    assert 0 < len(Vo) < len(V)
    np.testing.assert_array_equal(V2.cpu().numpy().view(np.uint64), Vo.view(np.uint64))
    np.testing.assert_array_equal(T2.cpu().numpy(), To)


row("trim_by_density",
    lambda mg, ms, d: _trim(ms, 4095),
    lambda mg, ms, d: _trim(ms, 4097))

# -- mesh clean-up ---------------------------------------------------------------------------------------------
COMPONENTS = t_clean.COMPONENTS


@functools.lru_cache(maxsize=None)
def _components_case(name, with_vertices):
    if name == "area_case":
        P, T, _ = cs.area_case()
        return P, T, len(P), oc.cluster_connected_triangles(T, len(P), P)
    T, nv = COMPONENTS[name]
    P = np.random.default_rng(5).normal(size=(nv, 3)) if with_vertices else None
    return P, T, nv, oc.cluster_connected_triangles(T, nv, P) if with_vertices else oc.cluster_connected_triangles(T, nv)


def _components(ms, name, with_vertices):
    P, T, nv, want = _components_case(name, with_vertices)
    if with_vertices:
        t_clean._same(t_clean._twice(lambda: ms.cluster_connected_triangles(P, T)), want)
    else:
        t_clean._same(t_clean._twice(lambda: ms.cluster_connected_triangles(None, T, n_vertices=nv)), want)


row("cluster_connected_triangles[areas]",
    lambda mg, ms, d: _components(ms, "area_case", True),
    lambda mg, ms, d: _components(ms, "strip_4097", True))

row("cluster_connected_triangles[no areas]",
    lambda mg, ms, d: _components(ms, "shared_edge", False),
    lambda mg, ms, d: _components(ms, "strip_4097", False))

row("remove_triangles_by_mask",
    lambda mg, ms, d: t_clean.test_remove_triangles_by_mask(ms, 1, "one"),
    lambda mg, ms, d: t_clean.test_remove_triangles_by_mask(ms, 4097, "alternating"))

row("remove_unreferenced_vertices",
    lambda mg, ms, d: t_clean.test_remove_unreferenced_vertices(ms, "holes_1"),
    lambda mg, ms, d: t_clean.test_remove_unreferenced_vertices(ms, "holes_4097"))

row("simplify_vertex_clustering",
    lambda mg, ms, d: t_clean.test_simplify(ms, "own_voxels"),
    lambda mg, ms, d: t_clean.test_simplify(ms, "strip_4097"))

# -- mesh writing ----------------------------------------------------------------------------------------------
_WRITE_MESHES = {"one": lambda: t_write.small_mesh(1), "fan": wo.fan_mesh,
                 "ring": lambda: wo.random_mesh(t_write.RING_T, nv=700, seed=11)}


@functools.lru_cache(maxsize=None)
def _write_case(name):
    """-> (P, T, triangle normals, vertex normals, {extension: the file's bytes})."""
    P, T = _WRITE_MESHES[name]()
    return P, T, pmo.triangle_normals(P, T), wo.vertex_normals(P, T), {e: t_write._want(e, P, T) for e in t_write.EXTS}


def _mesh_normals(ms, name, which):
    P, T, tn, vn, _ = _write_case(name)
    fn, ref = (ms.compute_triangle_normals, tn) if which == "triangle" else (ms.compute_vertex_normals, vn)
    a, b = (fn(*t_write._dev(P, T)).cpu().numpy() for _ in range(2))
    np.testing.assert_array_equal(t_write._bits(a), t_write._bits(b))
    np.testing.assert_array_equal(t_write._bits(a), t_write._bits(ref))


def _written(ms, d, name, ext, **kw):
    P, T, _, _, want = _write_case(name)
    assert t_write._written_twice(ms, d, ext, P, T, **kw) == want[ext]


for _which in ("triangle", "vertex"):
    row(f"compute_{_which}_normals",
        lambda mg, ms, d, w=_which: _mesh_normals(ms, "one", w),
        lambda mg, ms, d, w=_which: _mesh_normals(ms, "fan", w),
        lambda mg, ms, d, w=_which: _mesh_normals(ms, "ring", w))
for _ext in t_write.EXTS:
    row(f"write_triangle_mesh[{_ext}]",
        lambda mg, ms, d, e=_ext: _written(ms, d, "one", e),
        lambda mg, ms, d, e=_ext: _written(ms, d, "fan", e),
        lambda mg, ms, d, e=_ext: _written(ms, d, "ring", e, chunk_triangles=256))


# ---- the matrix ----------------------------------------------------------------------------------------------
def _poisoned(mg, ms, tmp_path, name, checks, byte, side):
    """Run the row's checks one by one with the pool poisoned; each must have drawn scratch -> bytes poisoned."""
    total = 0
    with mg.pool_poison(byte) as poison:
        for k, check in enumerate(checks):
            before = poison.bytes()
            if side:
                stream = torch.cuda.Stream()
                with torch.cuda.stream(stream):
                    check(mg, ms, tmp_path)
                stream.synchronize()
            else:
                check(mg, ms, tmp_path)
            grew = poison.bytes() - before
            assert grew > 0, f"{name}: check {k} took no scratch from the pool"
            total += grew
    return total


def test_every_required_wrapper_has_a_row_and_none_is_excused():
    for wrapper, rows in REQUIRED.items():
        assert rows and all(r in ROWS for r in rows), wrapper
    excused = {name.split("[")[0] for name, _, _ in NO_SCRATCH}
    assert all(why for _, why, _ in NO_SCRATCH)
    assert not excused & set(REQUIRED)
    assert not {name for name, _, _ in NO_SCRATCH} & set(ROWS)


@pytest.mark.parametrize("entry", NO_SCRATCH, ids=[e[0] for e in NO_SCRATCH])
def test_no_scratch_wrappers_take_none(mg, ms, entry):
    """The list is a condition too: armed, the call leaves the counter where it was."""
    _, _, call = entry
    with mg.pool_poison(0xFF) as poison:
        before = poison.bytes()
        call(mg, ms)
        torch.cuda.synchronize()
        assert poison.bytes() == before


@pytest.mark.parametrize("cond", CONDITIONS, ids=[c[0] for c in CONDITIONS])
@pytest.mark.parametrize("name", list(ROWS))
def test_result_does_not_depend_on_scratch_contents(mg, ms, tmp_path, name, cond):
    _, byte, side = cond
    t0 = time.perf_counter()
    total = _poisoned(mg, ms, tmp_path, name, ROWS[name], byte, side)
    print(f"{name} [{cond[0]}]: {len(ROWS[name])} cases, {total} bytes poisoned, {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("name", list(ROWS))
def test_small_call_on_the_large_calls_buffers(mg, ms, tmp_path, name):
    """The largest case and at once the smallest, both poisoned.  (The pool reuses a kept buffer only for a request
    of at least half its size, so the small call's buffers are the large call's only where their sizes are that
    close; what the item holds to is that the small result is right whatever the pool hands out after a large one.)"""
    checks = ROWS[name]
    total = _poisoned(mg, ms, tmp_path, name, (checks[-1], checks[0]), 0xFF, False)
    print(f"{name} [large then small]: {total} bytes poisoned")


# ---- the pool itself -----------------------------------------------------------------------------------------
def test_trim_releases_everything_once(mg):
    P, C, vs = mc.voxel_tile_edge(mc.RS_TILE + 1)
    Qe, Ce = mo.voxel_down_sample(P, C, vs)
    before = [t.cpu().numpy() for t in mg.voxel_down_sample(P, C, vs)]
    assert mg.pool_trim() > 0
    assert mg.pool_trim() == 0
    after = [t.cpu().numpy() for t in mg.voxel_down_sample(P, C, vs)]  # every buffer of this call is a fresh one
    for b, a, want in zip(before, after, (Qe, Ce)):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, want)
    assert mg.pool_trim() > 0


def test_poison_switch_arguments_and_counter(mg):
    import ctypes

    from structured_light_for_3d_model_replication_amd import _lib
    L = _lib.load()
    P, C, vs = mc.voxel_tile_edge(mc.KT + 1)
    seen = ctypes.c_int64(-1)
    assert L.sl_merge_pool_poison(-1, ctypes.byref(seen)) == _lib.SL_OK
    start = seen.value
    assert start >= 0
    for bad in (256, -2):
        seen.value = -7
        assert L.sl_merge_pool_poison(bad, ctypes.byref(seen)) == _lib.SL_EINVAL
        with pytest.raises(ValueError):
            mg.pool_poison(bad).__enter__()
    assert L.sl_merge_pool_poison(-1, None) == _lib.SL_OK  # NULL is allowed
    mg.voxel_down_sample(P, C, vs)  # disarmed (the refused values armed nothing): nothing is counted
    assert mg.pool_poison(0).bytes() == start
    counts = [start]
    for byte in (0xFF, 0x00):
        with mg.pool_poison(byte) as poison:
            assert L.sl_merge_pool_poison(256, None) == _lib.SL_EINVAL  # refused: it stays armed
            t_edges._check_voxel(mg, P, C, vs)
            counts.append(poison.bytes())
        assert poison.bytes() == counts[-1]  # disarmed: it reads the same
        mg.voxel_down_sample(P, C, vs)
        counts.append(poison.bytes())
    assert counts[0] < counts[1] == counts[2] < counts[3] == counts[4]
    with pytest.raises(RuntimeError, match="inside"):
        with mg.pool_poison(0xFF) as poison:
            raise RuntimeError("inside")
    mg.voxel_down_sample(P, C, vs)
    assert poison.bytes() == counts[-1]  # the block's exception disarmed it
    # reading the counter leaves the mode alone, and an inner block gives the outer one its mode back
    with mg.pool_poison(0x55) as outer:
        assert mg.pool_poison(0xFF).bytes() == counts[-1]  # an object that was never entered: still armed
        mg.voxel_down_sample(P, C, vs)
        a = outer.bytes()
        with mg.pool_poison(0xFF) as inner:
            mg.voxel_down_sample(P, C, vs)
        b = inner.bytes()
        mg.voxel_down_sample(P, C, vs)
        c = outer.bytes()
    mg.voxel_down_sample(P, C, vs)
    assert counts[-1] < a < b < c == outer.bytes()
