"""GPU mesh smoothing (csrc/slmeshsmooth.inl) against its CPU restatement (tests/meshsmooth_oracle.py): exact, and
every result computed twice and required to repeat."""
import numpy as np
import pytest
import torch

from tests import mesh_oracle as mo
from tests import meshsmooth_cases as cs
from tests import meshsmooth_oracle as so

pytestmark = pytest.mark.gpu

ADJACENCY = cs.adjacency_cases()


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


def _filter(ms, run, P=None, T=None):
    mesh, method, kw = cs.RUNS[run]
    if P is None:
        P, T = cs.MESHES[mesh]
    return getattr(ms, f"filter_smooth_{method}")(P, T, **kw)


# ---- adjacency ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ADJACENCY))
def test_adjacency(ms, name):
    T, nv = ADJACENCY[name]
    got = _twice(lambda: ms.adjacency_list(T, nv, boundary=True))
    _same(got, so.adjacency_list(T, nv, boundary=True))
    _same(_twice(lambda: ms.adjacency_list(T, nv)), got[:2])


@pytest.mark.parametrize("name", sorted(cs.BAD_INDEX_CASES))
def test_bad_indices_raise(ms, name):
    T, nv = cs.BAD_INDEX_CASES[name]
    P = np.zeros((nv, 3))
    with pytest.raises(IndexError, match="triangle index out of range"):
        ms.adjacency_list(T, nv)
    with pytest.raises(IndexError, match="triangle index out of range"):
        ms.adjacency_list(T, nv, boundary=True)
    for method in ("simple", "laplacian", "taubin"):
        with pytest.raises(IndexError, match="triangle index out of range"):
            getattr(ms, f"filter_smooth_{method}")(P, T)


def test_adjacency_accepts_tensors_and_leaves_them(ms):
    T, nv = ADJACENCY["strip_4097"]
    want = so.adjacency_list(T, nv, boundary=True)
    for t in (torch.from_numpy(T), torch.from_numpy(T).cuda(), torch.from_numpy(T.astype(np.int64)).cuda()):
        before = t.clone()
        _same(_twice(lambda: ms.adjacency_list(t, nv, boundary=True)), want)
        assert torch.equal(t, before)
    with pytest.raises(ValueError):
        ms.adjacency_list(T, -1)
    with pytest.raises(ValueError):
        ms.adjacency_list(T, 2 ** 31)
    with pytest.raises(ValueError):
        ms.adjacency_list(T[:, :2], nv)


# ---- the filters ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", sorted(cs.RUNS))
def test_filter(ms, run):
    got = _twice(lambda: (_filter(ms, run),))
    _same(got, (cs.reference(run),))


@pytest.mark.parametrize("run", ["hub_257-taubin-iterations=2", "noisy_sphere-simple-iterations=10",
                                 "sheet_9x7-laplacian-iterations=2-fixed_boundary=True", "noisy_sphere-taubin-iterations=0"])
def test_filter_accepts_tensors_and_leaves_them(ms, run):
    P, T = cs.MESHES[cs.RUNS[run][0]]
    want = (cs.reference(run),)
    for dev in ("cpu", "cuda"):
        Pt, Tt = torch.from_numpy(P.copy()).to(dev), torch.from_numpy(T.copy()).to(dev)
        out = _filter(ms, run, Pt, Tt)
        assert out.is_cuda and out.data_ptr() != Pt.data_ptr()          # new vertices, iterations = 0 included
        _same(_twice(lambda: (_filter(ms, run, Pt, Tt),)), want)
        np.testing.assert_array_equal(_np(Pt), P)                       # the input is unchanged
        np.testing.assert_array_equal(_np(Tt), T)
    _same((_np(_filter(ms, run, P, torch.from_numpy(T.astype(np.int64)).cuda())),), want)   # int64 indices too


def test_argument_errors(ms):
    P, T = cs.MESHES["coincident"]
    for method in ("simple", "laplacian", "taubin"):
        fn = getattr(ms, f"filter_smooth_{method}")
        with pytest.raises(ValueError):
            fn(P, T, -1)
        for v in (np.nan, np.inf, -np.inf):
            bad = P.copy()
            bad[2, 1] = v
            with pytest.raises(ValueError, match="non-finite"):
                fn(bad, T)
        with pytest.raises(ValueError):
            fn(P[:, :2], T)
    for v in (np.nan, np.inf):
        with pytest.raises(ValueError):
            ms.filter_smooth_laplacian(P, T, 1, v)
        with pytest.raises(ValueError):
            ms.filter_smooth_taubin(P, T, 1, v)
        with pytest.raises(ValueError):
            ms.filter_smooth_taubin(P, T, 1, 0.5, v)
    _same((_np(ms.filter_smooth_taubin(P, T, 1, 0.5, -0.53)),), (so.filter_smooth_taubin(P, T, 1),))  # still usable


def test_smooth_stats(ms):
    keys = {"keys_ms", "sort_ms", "csr_ms", "iterations_ms"}
    _filter(ms, "strip_4097-taubin-iterations=2")
    stats = ms.smooth_stats()
    assert set(stats) == keys and all(v > 0.0 for v in stats.values())
    ms.adjacency_list(*ADJACENCY["strip_4097"])
    stats = ms.smooth_stats()
    assert set(stats) == keys and stats["iterations_ms"] == 0.0 and stats["sort_ms"] > 0.0
    _filter(ms, "noisy_sphere-taubin-iterations=0")
    assert all(v == 0.0 for v in ms.smooth_stats().values())


# ---- scratch contents and streams -----------------------------------------------------------------------------
SMALL, LARGE = "sheet_9x7-taubin-iterations=2-fixed_boundary=True", "strip_4097-taubin-iterations=2"


def _check_run(ms, run):
    _same((_np(_filter(ms, run)),), (cs.reference(run),))


def _check_adjacency(ms, name):
    _same(tuple(_np(x) for x in ms.adjacency_list(*ADJACENCY[name], boundary=True)),
          so.adjacency_list(*ADJACENCY[name], boundary=True))


def test_result_does_not_depend_on_scratch_contents(ms, mg):
    """The pool's buffers filled with 0xFF before every use (a double reads as NaN, an index as -1): the same
    bits, for the small case, for a larger one, and for the small one served from what the larger one left."""
    with mg.pool_poison(0xFF) as poison:  # (disarmed again when the block ends, however it ends)
        for check, arg in ((_check_run, SMALL), (_check_run, LARGE), (_check_run, SMALL),
                           (_check_adjacency, "sheet_9x7"), (_check_adjacency, "strip_4097"),
                           (_check_adjacency, "sheet_9x7")):
            before = poison.bytes()
            check(ms, arg)
            assert poison.bytes() > before, "the call took no scratch from the pool"


def test_on_a_side_stream(ms):
    side = torch.cuda.Stream()
    for check, arg in ((_check_run, SMALL), (_check_run, LARGE), (_check_adjacency, "strip_4097")):
        with torch.cuda.stream(side):
            check(ms, arg)
        side.synchronize()


# ---- through the drop-ins -------------------------------------------------------------------------------------
def _read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def cloud(tmp_path_factory):
    """A sphere cloud with normals as a .ply -> (its directory, the file, the points and normals on the device)."""
    from structured_light_for_3d_model_replication_amd import ply
    d = tmp_path_factory.mktemp("meshsmooth")
    P, N = mo.sphere(6000, (0.1, -0.2, 0.3))
    src = str(d / "sphere.ply")
    ply.save_ply_open3d(P, np.zeros((len(P), 3), np.uint8), src, normals=N)
    c = ply.read_cloud_device(src)
    return d, src, c["points"], c["normals"]


def test_reconstruct_stl_smooths(ms, pr, cloud, capsys):
    d, src, P, N = cloud
    V, T, dens = ms.create_from_point_cloud_poisson(P, N, depth=5)
    V, T = ms.trim_by_density(V, T, dens, 0.02)
    L = pr.ProcessingLogic
    plain, by_hand, smooth, smooth_hand = (str(d / n) for n in ("plain.stl", "hand.stl", "smooth.stl", "smooth_hand.stl"))
    ms.write_triangle_mesh(by_hand, V, T)
    L.reconstruct_stl(src, plain, params={"depth": 5})
    assert capsys.readouterr().out.splitlines() == [
        f"[Recon] Loading {src}...", "[Recon] Poisson Reconstruction (depth=5)...",
        "[Recon] Computing normals and saving...", f"[Recon] Saved STL to {plain}"]
    assert _read(plain) == _read(by_hand)                                  # no keyword: today's file
    V5 = ms.filter_smooth_taubin(V, T, 5)
    ms.write_triangle_mesh(smooth_hand, V5, T)
    L.reconstruct_stl(src, smooth, params={"depth": 5}, smooth_iterations=5)
    assert capsys.readouterr().out.splitlines() == [
        f"[Recon] Loading {src}...", "[Recon] Poisson Reconstruction (depth=5)...",
        f"[Recon] Smoothing (taubin, 5 iterations): {len(V)} vertices",
        "[Recon] Computing normals and saving...", f"[Recon] Saved STL to {smooth}"]
    assert _read(smooth) == _read(smooth_hand) != _read(plain)
    np.testing.assert_array_equal(_np(V5), so.filter_smooth_taubin(_np(V), _np(T), 5))
    for name, kw, fn in (("simple.stl", {"smooth_method": "simple"}, ms.filter_smooth_simple),
                         ("fixed.stl", {"smooth_fixed_boundary": True},
                          lambda V, T, n: ms.filter_smooth_taubin(V, T, n, fixed_boundary=True))):
        out, hand = str(d / name), str(d / ("hand_" + name))
        L.reconstruct_stl(src, out, params={"depth": 5}, smooth_iterations=2, **kw)
        ms.write_triangle_mesh(hand, fn(V, T, 2), T)
        assert _read(out) == _read(hand)
    capsys.readouterr()
    for call in (lambda: L.reconstruct_stl(src, str(d / "never.stl"), params={"depth": 5}, smooth_method="nope"),
                 lambda: L.reconstruct_stl(src, str(d / "never.stl"), params={"depth": 5}, smooth_iterations=3,
                                           smooth_method="nope"),
                 lambda: L.mesh_360(src, str(d / "never.stl"), depth=5, smooth_iterations=3, smooth_method="nope")):
        with pytest.raises(ValueError, match="smooth_method"):
            call()
    assert not (d / "never.stl").exists()


def test_mesh_360_smooths(ms, mg, pr, cloud, capsys):
    """mesh_360 estimates and orients its own normals: the mesh it starts from is rebuilt with the calls it makes."""
    d, src, P, _ = cloud
    N = mg.estimate_normals(P, radius=0.1, max_nn=30)
    N = -ms.orient_normals_towards_camera_location(P, N, ms.get_center(P))
    V, T, dens = ms.create_from_point_cloud_poisson(P, N, depth=5)
    V, T = ms.trim_by_density(V, T, dens, 0.01)
    L = pr.ProcessingLogic
    plain, by_hand, smooth, smooth_hand = (str(d / n) for n in ("p360.ply", "h360.ply", "s360.ply", "sh360.ply"))
    ms.write_triangle_mesh(by_hand, V, T)
    L.mesh_360(src, plain, depth=5, orientation_mode="radial")
    assert _read(plain) == _read(by_hand)                                  # no keyword: today's file
    assert not any("Smoothing" in line for line in capsys.readouterr().out.splitlines())
    ms.write_triangle_mesh(smooth_hand, ms.filter_smooth_laplacian(V, T, 3), T)
    L.mesh_360(src, smooth, depth=5, orientation_mode="radial", smooth_iterations=3, smooth_method="laplacian")
    assert capsys.readouterr().out.splitlines()[-2:] == [
        f"[360 Mesh] Smoothing (laplacian, 3 iterations): {len(V)} vertices", f"[360 Mesh] Saved to {smooth}"]
    assert _read(smooth) == _read(smooth_hand) != _read(plain)
