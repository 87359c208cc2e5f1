"""GPU mesh clean-up (csrc/slmeshclean.inl) against its CPU restatement (tests/meshclean_oracle.py): exact, and
every result computed twice and required to repeat."""
import numpy as np
import pytest
import torch

from tests import mesh_oracle as mo
from tests import meshclean_cases as cs
from tests import meshclean_oracle as oc

pytestmark = pytest.mark.gpu

COMPONENTS = cs.components_cases()
SIMPLIFY = cs.simplify_cases()
UNREFERENCED = cs.unreferenced_cases()


@pytest.fixture(scope="module")
def ms():
    from structured_light_for_3d_model_replication_amd import mesh
    return mesh


@pytest.fixture(scope="module")
def pr():
    from structured_light_for_3d_model_replication_amd import processing
    return processing


def _np(x):
    return None if x is None else x.cpu().numpy()


def _twice(fn):
    """fn() twice -> the first result as NumPy arrays, after requiring the second to be identical."""
    a, b = [tuple(_np(x) for x in fn()) for _ in range(2)]
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.dtype == y.dtype
            np.testing.assert_array_equal(x, y)
    return a


def _same(got, want):
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if w is not None:
            assert g.dtype == w.dtype and g.shape == w.shape
            np.testing.assert_array_equal(g, w)


# ---- connected components -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(COMPONENTS))
def test_components(ms, name):
    T, nv = COMPONENTS[name]
    got = _twice(lambda: ms.cluster_connected_triangles(None, T, n_vertices=nv))
    _same(got, oc.cluster_connected_triangles(T, nv))


@pytest.mark.parametrize("name", ["strip_4097", "isolated_4097", "degenerate_aab", "t0"])
def test_components_with_vertices(ms, name):
    T, nv = COMPONENTS[name]
    P = np.random.default_rng(5).normal(size=(nv, 3))
    got = _twice(lambda: ms.cluster_connected_triangles(P, T))
    _same(got, oc.cluster_connected_triangles(T, nv, P))
    assert got[2] is not None and got[2].dtype == np.float64
    no_area = _twice(lambda: ms.cluster_connected_triangles(P, T, area=False))
    assert no_area[2] is None
    _same(no_area[:2], got[:2])


def test_component_areas(ms):
    P, T, sizes = cs.area_case()
    got = _twice(lambda: ms.cluster_connected_triangles(P, T))
    _same(got, oc.cluster_connected_triangles(T, len(P), P))
    assert got[1].tolist() == sizes
    stats = ms.cluster_stats()
    assert set(stats) == {"edge_keys_ms", "sort_ms", "union_ms", "flatten_rank_ms", "counts_ms", "areas_ms"}
    assert all(v > 0.0 for v in stats.values())
    ms.cluster_connected_triangles(P, T, area=False)
    assert ms.cluster_stats()["areas_ms"] == 0.0 and ms.cluster_stats()["sort_ms"] > 0.0


@pytest.mark.parametrize("name", sorted(cs.BAD_INDEX_CASES))
def test_bad_indices_raise(ms, name):
    T, nv = cs.BAD_INDEX_CASES[name]
    P = np.zeros((nv, 3))
    with pytest.raises(IndexError, match="triangle index out of range"):
        ms.cluster_connected_triangles(None, T, n_vertices=nv)
    with pytest.raises(IndexError, match="triangle index out of range"):
        ms.cluster_connected_triangles(P, T)
    with pytest.raises(IndexError, match="triangle index out of range"):
        ms.remove_unreferenced_vertices(P, T)
    with pytest.raises(IndexError, match="triangle index out of range"):
        ms.simplify_vertex_clustering(P, T, 1.0)
    with pytest.raises(IndexError, match="triangle index out of range"):
        ms.select_components(P, T, keep_largest=True)


def test_components_argument_errors(ms):
    T = COMPONENTS["t1"][0]
    with pytest.raises(ValueError):
        ms.cluster_connected_triangles(None, T)
    with pytest.raises(ValueError):
        ms.cluster_connected_triangles(np.zeros((3, 3)), T, n_vertices=4)
    with pytest.raises(ValueError):
        ms.cluster_connected_triangles(None, T, n_vertices=2 ** 31)
    bad = np.zeros((3, 3))
    bad[1, 2] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        ms.cluster_connected_triangles(bad, T)
    labels, counts, area = ms.cluster_connected_triangles(bad, T, area=False)      # the vertices are not read
    assert labels.tolist() == [0] and counts.tolist() == [1] and area is None


# ---- masks and unreferenced vertices --------------------------------------------------------------------------
@pytest.mark.parametrize("n", cs.MASK_SIZES)
@pytest.mark.parametrize("kind", cs.MASK_KINDS)
def test_remove_triangles_by_mask(ms, n, kind):
    P, T, m = cs.mask_case(n, kind)
    got = _twice(lambda: ms.remove_triangles_by_mask(P, T, m))
    _same(got, oc.remove_triangles_by_mask(P, T, m))
    if n:
        with pytest.raises(ValueError):
            ms.remove_triangles_by_mask(P, T, m[:-1])


@pytest.mark.parametrize("name", sorted(UNREFERENCED))
def test_remove_unreferenced_vertices(ms, name):
    P, T = UNREFERENCED[name]
    got = _twice(lambda: ms.remove_unreferenced_vertices(P, T))
    _same(got, oc.remove_unreferenced_vertices(P, T))


def test_select_components(ms):
    P, T, sizes = cs.area_case()
    for kw in ({"keep_largest": True}, {"min_triangles": 64}, {"min_triangles": 65, "keep_largest": True},
               {"min_triangles": 130}, {"min_triangles": 130, "keep_largest": True}, {}):
        got = _twice(lambda: ms.select_components(P, T, **kw))
        _same(got, oc.select_components(P, T, **kw))
    # a tie: the lowest label wins
    T2, nv = COMPONENTS["t2_apart"]
    P2 = np.arange(18, dtype=np.float64).reshape(6, 3)
    got = _twice(lambda: ms.select_components(P2, T2, keep_largest=True))
    _same(got, oc.select_components(P2, T2, keep_largest=True))
    np.testing.assert_array_equal(got[0], P2[:3])


# ---- vertex clustering ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SIMPLIFY))
def test_simplify(ms, name):
    P, T, vs = SIMPLIFY[name]
    got = _twice(lambda: ms.simplify_vertex_clustering(P, T, vs))
    _same(got, oc.simplify_vertex_clustering(P, T, vs))


@pytest.mark.parametrize("steps", [1.5, 2.0, 4.0])
def test_simplify_poisson_sphere(ms, steps):
    V, T, h = cs.poisson_sphere()
    got = _twice(lambda: ms.simplify_vertex_clustering(V, T, steps * h))
    _same(got, oc.simplify_vertex_clustering(V, T, steps * h))
    assert 0 < len(got[1]) < len(T)


def test_simplify_errors(ms):
    P, T, _ = SIMPLIFY["on_a_face"]
    for vs in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="voxel_size <= 0."):
            ms.simplify_vertex_clustering(P, T, vs)
    with pytest.raises(ValueError, match="voxel_size is too small."):
        ms.simplify_vertex_clustering(P, T, 1e-10)
    with pytest.raises(ValueError, match="2e6 voxels per axis"):
        ms.simplify_vertex_clustering(P, T, 1e-7)
    for v in (np.nan, np.inf):
        bad = P.copy()
        bad[2, 1] = v
        with pytest.raises(ValueError, match="non-finite"):
            ms.simplify_vertex_clustering(bad, T, 0.5)


# ---- through the drop-ins -------------------------------------------------------------------------------------
def _write_ply(path, P, N=None):
    from structured_light_for_3d_model_replication_amd import ply
    ply.save_ply_open3d(P, np.zeros((len(P), 3), np.uint8), str(path), normals=N)
    return str(path)


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _n_components(stl):
    """Of a binary STL: triangles that share two corner positions share an edge."""
    rec = np.frombuffer(stl[84:], dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]))
    corners, T = np.unique(rec["v"].reshape(-1, 3), axis=0, return_inverse=True)
    return len(oc.cluster_connected_triangles(T.reshape(-1, 3), len(corners))[1])


@pytest.fixture(scope="module")
def recon(ms, pr, tmp_path_factory):
    """The two-sphere cloud as a .ply with normals, the file today's reconstruct_stl path writes for it and the
    mesh (after the 2 % trim) it is made from -- the GPU's own, as the f32 FFT is not bit-pinned."""
    from structured_light_for_3d_model_replication_amd import ply
    d = tmp_path_factory.mktemp("meshclean")
    P, N = cs.two_spheres()
    src = _write_ply(d / "two.ply", P, N)
    cloud = ply.read_cloud_device(src)
    V, T, dens = ms.create_from_point_cloud_poisson(cloud["points"], cloud["normals"], depth=5)
    V, T = ms.trim_by_density(V, T, dens, 0.02)
    ms.write_triangle_mesh(str(d / "parent.stl"), V, T)
    return {"dir": d, "src": src, "V": _np(V), "T": _np(T), "h": float(mo.box(_np(cloud["points"]), 5)[1]),
            "parent": _read(d / "parent.stl")}


def test_reconstruct_stl_keeps_the_largest_component(pr, recon, capsys):
    d, src, V, T = recon["dir"], recon["src"], recon["V"], recon["T"]
    L = pr.ProcessingLogic
    plain, largest, by_size = (str(d / n) for n in ("plain.stl", "largest.stl", "by_size.stl"))
    L.reconstruct_stl(src, plain, params={"depth": 5})
    assert capsys.readouterr().out.splitlines() == [
        f"[Recon] Loading {src}...", "[Recon] Poisson Reconstruction (depth=5)...",
        "[Recon] Computing normals and saving...", f"[Recon] Saved STL to {plain}"]
    assert _read(plain) == recon["parent"] == mo.stl_bytes(V, T)           # no keyword: today's file
    assert _n_components(_read(plain)) == 2
    L.reconstruct_stl(src, largest, params={"depth": 5}, keep_largest_component=True)
    V1, T1 = oc.select_components(V, T, keep_largest=True)
    assert capsys.readouterr().out.splitlines() == [
        f"[Recon] Loading {src}...", "[Recon] Poisson Reconstruction (depth=5)...",
        f"[Recon] Selecting components: {len(T)} -> {len(T1)} triangles",
        "[Recon] Computing normals and saving...", f"[Recon] Saved STL to {largest}"]
    assert _read(largest) == mo.stl_bytes(V1, T1)
    assert 0 < len(T1) < len(T) and _n_components(_read(largest)) == 1
    L.reconstruct_stl(src, by_size, params={"depth": 5}, min_component_triangles=1000)
    assert _read(by_size) == _read(largest)


def test_reconstruct_stl_simplifies(pr, recon, capsys):
    d, src, V, T, h = recon["dir"], recon["src"], recon["V"], recon["T"], recon["h"]
    out = str(d / "coarse.stl")
    pr.ProcessingLogic.reconstruct_stl(src, out, params={"depth": 5}, keep_largest_component=True,
                                       simplify_voxel_size=2.0 * h)
    V1, T1 = oc.select_components(V, T, keep_largest=True)
    V2, T2 = oc.simplify_vertex_clustering(V1, T1, 2.0 * h)
    assert capsys.readouterr().out.splitlines()[2:4] == [
        f"[Recon] Selecting components: {len(T)} -> {len(T1)} triangles",
        f"[Recon] Vertex clustering (voxel_size={2.0 * h}): {len(T1)} -> {len(T2)} triangles"]
    assert _read(out) == mo.stl_bytes(V2, T2)
    assert 0 < len(T2) < len(T1) // 2
    only = str(d / "coarse_only.stl")
    pr.ProcessingLogic.reconstruct_stl(src, only, params={"depth": 5}, simplify_voxel_size=2.0 * h)
    assert _read(only) == mo.stl_bytes(*oc.simplify_vertex_clustering(V, T, 2.0 * h))


def test_mesh_360_cleans(ms, pr, recon, capsys):
    """mesh_360 estimates and orients its own normals: the mesh it starts from is rebuilt with the calls it makes."""
    from structured_light_for_3d_model_replication_amd import merge, ply
    d, src = recon["dir"], recon["src"]
    P = ply.read_cloud_device(src)["points"]
    N = merge.estimate_normals(P, radius=0.1, max_nn=30)
    N = -ms.orient_normals_towards_camera_location(P, N, ms.get_center(P))
    V, T, dens = ms.create_from_point_cloud_poisson(P, N, depth=5)
    V, T = ms.trim_by_density(V, T, dens, 0.01)
    ms.write_triangle_mesh(str(d / "parent360.stl"), V, T)
    V, T, h = _np(V), _np(T), float(mo.box(_np(P), 5)[1])
    L = pr.ProcessingLogic
    plain, clean = str(d / "plain360.stl"), str(d / "clean360.stl")
    L.mesh_360(src, plain, depth=5, orientation_mode="radial")
    assert _read(plain) == _read(d / "parent360.stl") == mo.stl_bytes(V, T)
    lines = capsys.readouterr().out.splitlines()
    assert lines[-2:] == ["[360 Mesh] Trimming low density vertices (threshold=0.01)...", f"[360 Mesh] Saved to {plain}"]
    L.mesh_360(src, clean, depth=5, orientation_mode="radial", keep_largest_component=True,
               min_component_triangles=10, simplify_voxel_size=2.0 * h)
    V1, T1 = oc.select_components(V, T, keep_largest=True, min_triangles=10)
    V2, T2 = oc.simplify_vertex_clustering(V1, T1, 2.0 * h)
    assert capsys.readouterr().out.splitlines()[-3:] == [
        f"[360 Mesh] Selecting components: {len(T)} -> {len(T1)} triangles",
        f"[360 Mesh] Vertex clustering (voxel_size={2.0 * h}): {len(T1)} -> {len(T2)} triangles",
        f"[360 Mesh] Saved to {clean}"]
    assert _read(clean) == mo.stl_bytes(V2, T2)
    assert 0 < len(T2) < len(T1) <= len(T)
    assert len(oc.cluster_connected_triangles(T1, len(V1))[1]) == 1
