"""GPU mesh checks (csrc/slmeshcheck.inl) against their CPU restatement (tests/meshcheck_oracle.py): exact, dtype and
shape included, and every result computed twice and required to repeat."""
import numpy as np
import pytest
import torch

from tests import mesh_oracle as mo
from tests import meshcheck_cases as kc
from tests import meshcheck_oracle as ko
from tests import meshclean_cases as mc
from tests import meshclean_oracle as mco

pytestmark = pytest.mark.gpu

CASES = kc.cases()
PLAIN = sorted(n for n in CASES if not n.endswith("_shuffled"))
IDX = "triangle index out of range"


@pytest.fixture(scope="module")
def ms():
    from structured_light_for_3d_model_replication_amd import mesh
    return mesh


@pytest.fixture(scope="module")
def mg():
    from structured_light_for_3d_model_replication_amd import merge
    return merge


@pytest.fixture(scope="module")
def pr():
    from structured_light_for_3d_model_replication_amd import processing
    return processing


def _np(x):
    return x.cpu().numpy()


def _twice(fn):
    """fn() twice -> the first result as NumPy arrays, after requiring the second to be identical."""
    a, b = [tuple(_np(x) for x in fn()) for _ in range(2)]
    for x, y in zip(a, b):
        assert x.dtype == y.dtype
        np.testing.assert_array_equal(x, y)
    return a


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        np.testing.assert_array_equal(g, w)


def _same_dict(got, want):
    assert got == want
    assert {k: type(v) for k, v in got.items()} == {k: type(v) for k, v in want.items()}


def _check_twice(ms, P, T, nv):
    a, b = (ms.check(P, T, n_vertices=nv) for _ in range(2))
    _same_dict(a, b)
    return a


def _lists(ms, T, nv):
    return (ms.get_non_manifold_edges(None, T, n_vertices=nv), ms.get_non_manifold_edges(None, T, False, n_vertices=nv),
            ms.get_non_manifold_vertices(None, T, n_vertices=nv))


# ---- every case against the oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_check(ms, name):
    P, T, nv = CASES[name]
    _same_dict(_check_twice(ms, P, T, nv), kc.reference(name, "check"))


@pytest.mark.parametrize("name", sorted(CASES))
def test_lists(ms, name):
    _, T, nv = CASES[name]
    _same(_twice(lambda: _lists(ms, T, nv)),
          (kc.reference(name, "edges"), kc.reference(name, "edges_closed"), kc.reference(name, "vertices")))


@pytest.mark.parametrize("name", sorted(CASES))
def test_orient_triangles(ms, name):
    _, T, nv = CASES[name]
    want, want_ok = kc.reference(name, "orient")
    flags = []

    def run():
        out, ok = ms.orient_triangles(None, T, n_vertices=nv)
        flags.append(ok)
        return (out,)
    got = _twice(run)
    assert flags == [want_ok, want_ok] and type(flags[0]) is bool
    _same(got, (want,))
    after = ms.check(None, got[0], n_vertices=nv)
    if want_ok:
        assert after["inconsistent_edges"] == 0 and after["orientable"]
    else:
        np.testing.assert_array_equal(got[0], T)


@pytest.mark.parametrize("name", PLAIN)
def test_views_and_removals(ms, name):
    P, T, nv = CASES[name]
    c = kc.reference(name, "check")
    kw = {"n_vertices": nv}
    assert ms.is_edge_manifold(P, T, **kw) is c["edge_manifold"]
    assert ms.is_edge_manifold(P, T, allow_boundary_edges=False, **kw) is c["edge_manifold_closed"]
    assert ms.is_vertex_manifold(P, T, **kw) is c["vertex_manifold"]
    assert ms.is_orientable(P, T, **kw) is c["orientable"]
    assert ms.is_watertight(P, T, **kw) is c["watertight"]
    _same(_twice(lambda: (ms.remove_degenerate_triangles(P, T, **kw)[1],)), (kc.reference(name, "degenerate"),))
    _same(_twice(lambda: (ms.remove_duplicated_triangles(P, T, **kw)[1],)), (kc.reference(name, "duplicated"),))
    if P is not None:
        assert ms.get_surface_area(P, T) == c["area"]
        if c["watertight"]:
            assert ms.get_volume(P, T) == c["volume"] and ms.get_volume(P, T, signed=True) == c["signed_volume"]
        else:
            with pytest.raises(ValueError, match="not watertight"):
                ms.get_volume(P, T)


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_remove_duplicated_around_the_sort_tile(ms, n):
    """meshclean_cases.live_case: duplicates n - 1 rows apart and rotations next to each other, on exactly n rows."""
    P, T, _ = mc.live_case(n)
    want = ko.remove_duplicated_triangles(T, len(P))
    assert len(want) < n
    _same(_twice(lambda: (ms.remove_duplicated_triangles(P, T)[1],)), (want,))
    _same((_np(ms.remove_degenerate_triangles(P, T)[1]),), (T,))


def test_is_watertight_has_no_self_intersection_test(ms):
    P, T, _ = CASES["cube"]
    assert ms.is_watertight(P, T, check_self_intersection=False) is True
    with pytest.raises(NotImplementedError):
        ms.is_watertight(P, T, check_self_intersection=True)


# ---- errors ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(kc.BAD_INDEX_CASES))
def test_bad_indices_raise(ms, name):
    T, nv = kc.BAD_INDEX_CASES[name]
    P = np.zeros((nv, 3))
    for fn in (ms.check, ms.get_non_manifold_edges, ms.get_non_manifold_vertices, ms.is_edge_manifold,
               ms.is_vertex_manifold, ms.is_orientable, ms.is_watertight, ms.orient_triangles, ms.get_surface_area,
               ms.get_volume, ms.remove_degenerate_triangles, ms.remove_duplicated_triangles):
        with pytest.raises(IndexError, match=IDX):
            fn(P, T)
    with pytest.raises(IndexError, match=IDX):
        ms.check(None, T, n_vertices=nv)


def test_non_finite_vertices_raise(ms):
    P, T, _ = CASES["cube"]
    for v in (np.nan, np.inf, -np.inf):
        bad = P.copy()
        bad[7, 1] = v        # vertex 7: the last
        for fn in (ms.check, ms.get_surface_area, ms.get_volume):
            with pytest.raises(ValueError, match="non-finite"):
                fn(bad, T)
        assert ms.is_watertight(bad, T) is True      # the topology needs no coordinates
    assert ms.get_volume(P, T) == 1.0                  # still usable


@pytest.mark.parametrize("name", ["sheet_9x7", "strip_257", "cube_half_flipped", "book_3", "two_tetrahedra_one_vertex",
                                  "klein_8x9", "mobius_5"])
def test_get_volume_raises_unless_watertight(ms, name):
    P, T, nv = CASES[name]
    P = np.random.default_rng(0).normal(size=(nv, 3)) if P is None else P
    with pytest.raises(ValueError, match="not watertight"):
        ms.get_volume(P, T)
    with pytest.raises(ValueError, match="not watertight"):
        ms.get_volume(P, T, signed=True)


def test_argument_errors(ms):
    P, T, nv = CASES["cube"]
    with pytest.raises(ValueError):
        ms.check(None, T)
    with pytest.raises(ValueError):
        ms.check(P, T, n_vertices=nv + 1)
    with pytest.raises(ValueError):
        ms.check(None, T, n_vertices=2 ** 31)
    with pytest.raises(ValueError):
        ms.check(None, T[:, :2], n_vertices=nv)
    with pytest.raises(ValueError):
        ms.check(P[:, :2], T)


# ---- tensors, streams, scratch, stats -------------------------------------------------------------------------
def _everything(ms, P, T, nv):
    """Every array result of one mesh."""
    return (*_lists(ms, T, nv), ms.orient_triangles(P, T, n_vertices=nv)[0],
            ms.remove_degenerate_triangles(P, T, n_vertices=nv)[1], ms.remove_duplicated_triangles(P, T, n_vertices=nv)[1])


def _want(name):
    return tuple(kc.reference(name, w) if w != "orient" else kc.reference(name, w)[0]
                 for w in ("edges", "edges_closed", "vertices", "orient", "degenerate", "duplicated"))


def _check_case(ms, name):
    P, T, nv = CASES[name]
    _same_dict(ms.check(P, T, n_vertices=nv), kc.reference(name, "check"))
    _same(tuple(_np(x) for x in _everything(ms, P, T, nv)), _want(name))


@pytest.mark.parametrize("name", ["torus_64x65_half_flipped", "repeats_mixed", "two_cones_one_apex"])
def test_accepts_tensors_and_leaves_them(ms, name):
    P, T, nv = CASES[name]
    P = np.zeros((nv, 3)) if P is None else P
    want_check = ko.check(P, T)
    for dev, dtype in (("cpu", torch.int32), ("cuda", torch.int32), ("cuda", torch.int64)):
        Pt, Tt = torch.from_numpy(P.copy()).to(dev), torch.from_numpy(T.copy()).to(dev, dtype)
        _same_dict(ms.check(Pt, Tt), want_check)
        out = _everything(ms, Pt, Tt, nv)
        assert all(x.is_cuda and x.dtype == torch.int32 for x in out)
        assert all(x.data_ptr() != Tt.data_ptr() for x in out)
        _same(tuple(_np(x) for x in out), _want(name))
        np.testing.assert_array_equal(_np(Pt), P)                       # the inputs are unchanged
        np.testing.assert_array_equal(_np(Tt), T)
    V2, T2 = ms.remove_degenerate_triangles(torch.from_numpy(P).cuda(), T)
    assert V2.is_cuda and V2.shape == P.shape                            # the vertices stay


SMALL, LARGE = "repeats_mixed", "torus_3x1366_half_flipped"


def test_result_does_not_depend_on_scratch_contents(ms, mg):
    """The pool's buffers filled with 0xFF before every use: the same results, for a small case, a larger one, and
    the small one served from what the larger one left."""
    with mg.pool_poison(0xFF) as poison:
        for name in (SMALL, LARGE, SMALL):
            before = poison.bytes()
            _check_case(ms, name)
            assert poison.bytes() > before, "the call took no scratch from the pool"


def test_on_a_side_stream(ms):
    side = torch.cuda.Stream()
    for name in (SMALL, LARGE, "mobius_4097"):
        with torch.cuda.stream(side):
            _check_case(ms, name)
        side.synchronize()


def test_check_stats(ms):
    keys = {"side_keys_ms", "sort_ms", "classify_ms", "corners_ms", "parity_ms", "flips_ms", "measure_ms"}
    P, T, nv = CASES["torus_64x65"]
    ms.orient_triangles(P, T)
    s = ms.check_stats()
    assert set(s) == keys and s["measure_ms"] == 0.0 and all(v > 0.0 for k, v in s.items() if k != "measure_ms")
    ms.is_watertight(P, T)
    s = ms.check_stats()
    assert s["flips_ms"] == 0.0 and s["sort_ms"] > 0.0       # no flips were asked for
    ms.get_surface_area(P, T)
    s = ms.check_stats()
    assert s["measure_ms"] > 0.0 and s["sort_ms"] == 0.0
    ms.check(None, CASES["none"][1], n_vertices=5)
    assert all(v == 0.0 for v in ms.check_stats().values())


# ---- the library's own meshes ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def own_meshes(ms, mg):
    """name -> (vertices, triangles) as NumPy: the depth-6 Poisson sphere untrimmed, trimmed at 2 %, clustered at 2 h,
    and the ball-pivoted 1500-point sphere."""
    V, T, h = mc.poisson_sphere()
    out = {"poisson": (V, T)}
    P, N = mo.sphere(20000, (0.1, -0.2, 0.3))
    Vg, Tg, dens = ms.create_from_point_cloud_poisson(P, N, depth=6)
    out["trimmed"] = tuple(_np(x) for x in ms.trim_by_density(Vg, Tg, dens, 0.02))
    out["clustered"] = tuple(_np(x) for x in ms.simplify_vertex_clustering(V, T, 2.0 * h))
    Q = np.random.default_rng(1).normal(size=(1500, 3))
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    d = float(mg.compute_nearest_neighbor_distance(Q).mean())
    out["ball_pivoted"] = tuple(_np(x) for x in ms.create_from_point_cloud_ball_pivoting(Q, Q.copy(), [d, 2 * d, 4 * d]))
    return out


@pytest.mark.parametrize("name", ["poisson", "trimmed", "clustered", "ball_pivoted"])
def test_own_meshes(ms, own_meshes, name):
    V, T = own_meshes[name]
    nv = len(V)
    assert len(T) > 1000
    _same_dict(_check_twice(ms, V, T, nv), ko.check(V, T))
    _same(_twice(lambda: _lists(ms, T, nv)), (ko.get_non_manifold_edges(T, nv), ko.get_non_manifold_edges(T, nv, False),
                                              ko.get_non_manifold_vertices(T, nv)))
    want, ok = ko.orient_triangles(T, nv)
    got, got_ok = ms.orient_triangles(V, T)
    assert got_ok is ok
    _same((_np(got),), (want,))


# ---- through the drop-ins -------------------------------------------------------------------------------------
def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _stl_mesh(path):
    """A binary STL's triangles with coincident corners welded -> (vertices f64, triangles int32)."""
    raw = _read(path)
    n = int(np.frombuffer(raw[80:84], "<u4")[0])
    rec = np.frombuffer(raw[84:], dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]), count=n)
    pts = rec["v"].reshape(-1, 3)
    uniq, inv = np.unique(pts, axis=0, return_inverse=True)
    return uniq.astype(np.float64), inv.reshape(-1, 3).astype(np.int32)


@pytest.fixture(scope="module")
def cloud(tmp_path_factory):
    from structured_light_for_3d_model_replication_amd import ply
    d = tmp_path_factory.mktemp("meshcheck")
    P, N = mo.sphere(6000, (0.1, -0.2, 0.3))
    src = str(d / "sphere.ply")
    ply.save_ply_open3d(P, np.zeros((len(P), 3), np.uint8), src, normals=N)
    c = ply.read_cloud_device(src)
    return d, src, c["points"], c["normals"]


def _line(out, tag):
    lines = [x for x in out.splitlines() if x.startswith(tag)]
    assert len(lines) == 1
    return lines[0]


def _expected_check_line(tag, c):
    yes = lambda b: "yes" if b else "no"  # noqa: E731
    return (f"[{tag}] Mesh check: {c['vertices']} vertices, {c['triangles']} triangles, {c['boundary_edges']} boundary "
            f"edges, {c['non_manifold_edges']} non-manifold edges, {c['non_manifold_vertices']} non-manifold vertices, "
            f"orientable {yes(c['orientable'])}, watertight {yes(c['watertight'])}, area {c['area']!r}"
            + ("" if c["volume"] is None else f", volume {c['volume']!r}"))


def test_reconstruct_stl_checks_and_repairs(ms, pr, cloud, capsys):
    d, src, P, N = cloud
    L = pr.ProcessingLogic
    plain, off, on = (str(d / n) for n in ("plain.stl", "off.stl", "on.stl"))
    L.reconstruct_stl(src, plain, params={"depth": 5})
    out_plain = capsys.readouterr().out
    L.reconstruct_stl(src, off, params={"depth": 5}, check_mesh=False, repair_mesh=False)
    out_off = capsys.readouterr().out
    assert _read(off) == _read(plain)                                   # both off: today's file and today's prints
    assert out_off == out_plain.replace(plain, off)
    assert "Mesh check" not in out_plain and "Repair" not in out_plain
    L.reconstruct_stl(src, on, params={"depth": 5}, check_mesh=True, repair_mesh=True)
    out_on = capsys.readouterr().out
    # the mesh the drop-in wrote, rebuilt with the calls it makes
    V, T, dens = ms.create_from_point_cloud_poisson(P, N, depth=5)
    V, T = ms.trim_by_density(V, T, dens, 0.02)
    Vn, Tn = _np(V), _np(T)
    T1 = ko.remove_degenerate_triangles(Tn, len(Vn))
    T2 = ko.remove_duplicated_triangles(T1, len(Vn))
    T3, orientable = ko.orient_triangles(T2, len(Vn))
    flipped = int((T3 != T2).any(1).sum()) if orientable else 0
    c = ko.check(Vn, T3)
    outward = bool(c["watertight"] and c["signed_volume"] < 0.0)
    if outward:
        T3 = np.ascontiguousarray(T3[:, [0, 2, 1]])
    V4, T4 = mco.remove_unreferenced_vertices(Vn, T3)
    yes = lambda b: "yes" if b else "no"  # noqa: E731
    assert _line(out_on, "[Recon] Repair:") == (
        f"[Recon] Repair: {len(Tn) - len(T1)} degenerate and {len(T1) - len(T2)} duplicated triangles removed, "
        f"{flipped} flipped (orientable: {yes(orientable)}), turned outward: {yes(outward)}, "
        f"{len(Vn) - len(V4)} unreferenced vertices removed")
    assert _line(out_on, "[Recon] Mesh check:") == _expected_check_line("Recon", ko.check(V4, T4))
    lines = out_on.splitlines()
    assert lines.index(_line(out_on, "[Recon] Repair:")) < lines.index(_line(out_on, "[Recon] Mesh check:")) \
        < lines.index("[Recon] Computing normals and saving...")
    assert _read(on) == mo.stl_bytes(V4, T4)
    # the counts of the line are those of the file: an STL holds the triangles, welding its corners gives the edges
    Vw, Tw = _stl_mesh(on)
    w, m = ko.check(Vw, Tw), ko.check(V4, T4)
    if len(Vw) == len(V4):       # no two vertices fell on one float32 position
        for k in ("triangles", "boundary_edges", "non_manifold_edges", "non_manifold_vertices", "orientable", "watertight"):
            assert w[k] == m[k]
    # check alone: the unrepaired mesh, the file of a plain call
    only = str(d / "only.stl")
    L.reconstruct_stl(src, only, params={"depth": 5}, check_mesh=True)
    out_only = capsys.readouterr().out
    assert _read(only) == _read(plain) and "Repair" not in out_only
    assert _line(out_only, "[Recon] Mesh check:") == _expected_check_line("Recon", ko.check(Vn, Tn))


def test_mesh_360_checks_and_repairs(ms, mg, pr, cloud, capsys):
    d, src, P, _ = cloud
    L = pr.ProcessingLogic
    plain, off, on = (str(d / n) for n in ("p360.ply", "o360.ply", "c360.ply"))
    L.mesh_360(src, plain, depth=5, orientation_mode="radial")
    out_plain = capsys.readouterr().out
    L.mesh_360(src, off, depth=5, orientation_mode="radial", check_mesh=False, repair_mesh=False)
    assert _read(off) == _read(plain) and capsys.readouterr().out == out_plain.replace(plain, off)
    L.mesh_360(src, on, depth=5, orientation_mode="radial", check_mesh=True, repair_mesh=True)
    out_on = capsys.readouterr().out
    N = mg.estimate_normals(P, radius=0.1, max_nn=30)
    N = -ms.orient_normals_towards_camera_location(P, N, ms.get_center(P))
    V, T, dens = ms.create_from_point_cloud_poisson(P, N, depth=5)
    V, T = ms.trim_by_density(V, T, dens, 0.01)
    Vn, Tn = _np(V), _np(T)
    T2 = ko.remove_duplicated_triangles(ko.remove_degenerate_triangles(Tn, len(Vn)), len(Vn))
    T3, _ = ko.orient_triangles(T2, len(Vn))
    c = ko.check(Vn, T3)
    if c["watertight"] and c["signed_volume"] < 0.0:
        T3 = np.ascontiguousarray(T3[:, [0, 2, 1]])
    V4, T4 = mco.remove_unreferenced_vertices(Vn, T3)
    assert _line(out_on, "[360 Mesh] Repair:").startswith("[360 Mesh] Repair: ")
    assert _line(out_on, "[360 Mesh] Mesh check:") == _expected_check_line("360 Mesh", ko.check(V4, T4))
