"""Consistent tangent-plane normal orientation on the GPU (csrc/slorient.inl,
mesh.orient_normals_consistent_tangent_plane) against tests/orient_oracle.py.
The graph is the GPU's own sl_radius_search output (pinned bit for bit in
test_gpu_registration.py), handed to the oracle as it is; every case compares
the normals, the sorted tree slots and the component count exactly.  Then the
``tangent_planes`` keyword of the ``processing`` drop-ins."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import orient_oracle as oo

pytestmark = pytest.mark.gpu


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


def _signs(n, seed):
    return np.random.default_rng(seed).choice([-1.0, 1.0], size=(n, 1))


def _same(ms, mg, P, N, radius, k):
    """Run both on the GPU's graph; -> (normals, info, the graph)."""
    idx, _, cnt = mg.radius_search(P, radius, k)
    idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
    got, info = ms.orient_normals_mst(P, N, idx, cnt)
    got2, info2 = ms.orient_normals_consistent_tangent_plane(P, N, k, radius=radius, info=True)
    exp, tree, comps = oo.orient(P, N, idx, cnt)
    got = got.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == np.shape(N)
    assert info["components"] == comps
    np.testing.assert_array_equal(info["tree_slots"].cpu().numpy(), tree)
    np.testing.assert_array_equal(got, exp)
    np.testing.assert_array_equal(np.abs(got), np.abs(N))
    # the public entry builds the same graph itself
    assert torch.equal(got2.cpu(), torch.from_numpy(got)) and info2["components"] == comps
    assert torch.equal(info2["tree_slots"], info["tree_slots"])
    return got, info, (idx, cnt)


# radius 0.3 at 2000 points and 0.1 at 20 000 hold about 36 points each: k = 100 leaves cnt < k on most rows
# (rows longer than a wave), k = 12 and k = 3 cut every row; 20 000 points are 79 workgroups of vertices
@pytest.mark.parametrize("k", [12, 100, 3])
@pytest.mark.parametrize("n,radius", [(2000, 0.3), (20000, 0.1)])
def test_torus(ms, mg, n, radius, k):
    P, out = oo.torus(n, n + k)
    N = out * _signs(n, k)
    got, info, (_, cnt) = _same(ms, mg, P, N, radius, k)
    if k == 100:
        assert (cnt < k).mean() > 0.5 and cnt.max() > 64
    if k == 3:
        assert info["components"] > 1
    else:
        assert info["components"] == 1 and len(info["tree_slots"]) == n - 1
        assert oo.agreement(got, out) == 1.0
        assert oo.agreement(oo.radial(P, N), out) < 0.8


def test_all_ties_lattice(ms, mg):
    g = np.stack(np.meshgrid(np.arange(30.0), np.arange(30.0), indexing="ij"), -1).reshape(-1, 2)
    P = np.concatenate([g, np.full((900, 1), 0.25)], 1)
    N = np.zeros((900, 3))
    N[:, 2] = _signs(900, 5)[:, 0]
    got, info, _ = _same(ms, mg, P, N, 1.5, 9)  # every weight is 0: slot order alone; every z equal: root 0
    assert info["components"] == 1
    np.testing.assert_array_equal(got, np.broadcast_to([0.0, 0.0, 1.0], (900, 3)))
    # one round hooks everything into long chains, which the jumps then flatten (how many launches that takes
    # depends on what a launch sees of its own writes; one that changes words and one that does not are certain)
    assert info["rounds"] >= 1 and max(info["jumps"]) >= 2


def test_chain(ms, mg):
    n = 3000
    P = np.zeros((n, 3))
    P[:, 0] = np.arange(n)
    a = np.random.default_rng(8).random(n) * 2.0 * np.pi
    N = np.stack([np.zeros(n), np.cos(a), np.sin(a)], 1)
    _, info, _ = _same(ms, mg, P, N, 1.5, 3)  # the tree is the chain itself: depth n
    assert info["components"] == 1


def test_components(ms, mg):
    P1, out1 = oo.torus(1500, 21)
    P2, out2 = oo.torus(1500, 22, centre=(5.0, 0.0, 0.0))
    P = np.concatenate([P1, P2, [[2.5, 0.0, 7.0]]])
    N = np.concatenate([out1 * _signs(1500, 1), -out2, [[0.0, 0.0, -1.0]]])
    got, info, _ = _same(ms, mg, P, N, 0.35, 12)
    assert info["components"] == 3
    np.testing.assert_array_equal(got[-1], [0.0, 0.0, 1.0])
    assert oo.agreement(got[:1500], out1) == 1.0 and oo.agreement(got[1500:3000], out2) == 1.0


def test_degenerate_values(ms, mg):
    rng = np.random.default_rng(13)
    P = rng.random((64, 3))
    N = rng.normal(size=(64, 3))
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    N[0], N[1] = [1.0, 0.0, 0.0], [0.0, -1.0, 0.0]  # exactly orthogonal: dot 0, no flip
    c = rng.normal(size=(4000, 3))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    over = c[(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2] > 1.0]
    assert len(over)  # a unit vector whose computed |n . n| exceeds 1 by an ulp: the weight is clamped to 0
    N[2], N[3] = over[0], -over[0]
    N[4] = 0.0  # a zero normal
    P[0], P[1] = [0.5, 0.5, 0.5], [0.5, 0.5, 0.51]
    P[2], P[3] = [0.2, 0.2, 0.2], [0.2, 0.2, 0.21]
    P[6] = P[7] = P[5]  # duplicate points
    for k in (2, 8):
        _same(ms, mg, P, N, 0.5, k)
    slot, _, _, w, _ = oo.edges(N[2:4], np.array([[0, 1], [1, 0]]), np.array([2, 2]))
    assert (w == 0.0).all()


def test_edges_of_the_domain(ms, mg):
    e = np.zeros((0, 3))
    got, info = ms.orient_normals_consistent_tangent_plane(e, e, 5, radius=1.0, info=True)
    assert tuple(got.shape) == (0, 3) and info["components"] == 0 and len(info["tree_slots"]) == 0
    got, info = ms.orient_normals_consistent_tangent_plane(np.array([[1.0, 2.0, 3.0]]), np.array([[0.6, 0.0, -0.8]]),
                                                           5, radius=1.0, info=True)
    np.testing.assert_array_equal(got.cpu().numpy(), [[-0.6, -0.0, 0.8]])
    assert info["components"] == 1 and len(info["tree_slots"]) == 0
    # k = 1: self only, every point its own component, the sign by its own nz
    rng = np.random.default_rng(3)
    P, N = rng.random((777, 3)), rng.normal(size=(777, 3))
    N[::5, 2] = 0.0
    got, info, _ = _same(ms, mg, P, N, 0.5, 1)
    assert info["components"] == 777 and len(info["tree_slots"]) == 0
    np.testing.assert_array_equal(got, np.where(N[:, 2:3] < 0.0, -N, N))
    with pytest.raises(ValueError):
        ms.orient_normals_consistent_tangent_plane(P, N[:-1], 5, radius=1.0)
    with pytest.raises(ValueError):
        ms.orient_normals_mst(P, N, np.zeros((776, 2), np.int32), np.zeros(777, np.int32))


def test_bad_arguments_are_rejected_before_any_launch(ms, mg):
    eng = mg._engine(None)
    buf = torch.zeros(64, dtype=torch.float64, device=eng.device)
    ibuf = torch.zeros(64, dtype=torch.int32, device=eng.device)
    nt, nc = ctypes.c_int64(), ctypes.c_int64()

    def call(xyz, nrm, n, idx, cnt, k, pnt=ctypes.byref(nt), pnc=ctypes.byref(nc)):
        ms._call(eng, "sl_orient_normals_mst", xyz, nrm, n, idx, cnt, k, None, pnt, pnc)

    b, i = buf.data_ptr(), ibuf.data_ptr()
    with pytest.raises(ValueError, match=r"n \* k must be below 2\^32"):
        call(b, b, 1 << 26, i, i, 64)  # only the sizes are read
    with pytest.raises(ValueError, match=r"n \* k must be below 2\^32"):
        call(b, b, (1 << 31) - 1, i, i, 3)
    with pytest.raises(ValueError, match="2\\^31"):
        call(b, b, 1 << 31, i, i, 1)
    for args in [(b, b, 4, i, i, 0), (None, b, 4, i, i, 2), (b, None, 4, i, i, 2), (b, b, 4, None, i, 2),
                 (b, b, 4, i, None, 2), (b, b, -1, i, i, 2), (b, b, 4, i, i, 2, None), (b, b, 4, i, i, 2,
                                                                                       ctypes.byref(nt), None)]:
        with pytest.raises(ValueError, match="bad sizes or NULL"):
            call(*args)
    call(None, None, 0, None, None, 3)  # n = 0 succeeds and produces nothing
    assert nt.value == 0 and nc.value == 0


def test_run_to_run(ms, mg):
    P, out = oo.torus(20000, 77)
    N = out * _signs(20000, 77)
    idx, _, cnt = mg.radius_search(P, 0.1, 12)
    a, ia = ms.orient_normals_mst(P, N, idx, cnt)
    b, ib = ms.orient_normals_mst(P, N, idx, cnt)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert torch.equal(ia["tree_slots"], ib["tree_slots"]) and ia["components"] == ib["components"]
    assert ia["rounds"] == ib["rounds"] >= 2


def test_torus_through_estimate_normals(ms, mg):
    P, out = oo.torus(2000, 0)
    N = mg.estimate_normals(P, 0.3, 12)
    got, info = ms.orient_normals_consistent_tangent_plane(P, N, 12, radius=0.3, info=True)
    assert info["components"] == 1
    assert torch.equal(N, mg.estimate_normals(P, 0.3, 12))  # the input is left alone
    assert oo.agreement(got.cpu().numpy(), out) == 1.0
    share = oo.agreement(oo.radial(P, N.cpu().numpy()), out)
    print(f"radial orientation: {100 * share:.1f} % of the torus")
    assert share < 0.8


# ---- the drop-ins -------------------------------------------------------------------------------------------
def _write_ply(path, P):
    from structured_light_for_3d_model_replication_amd import ply
    ply.save_ply_open3d(P, np.zeros((len(P), 3), np.uint8), str(path))
    return str(path)


def _stl_triangles(path):
    n = int(np.frombuffer(open(path, "rb").read()[80:84], dtype="<u4")[0])
    assert os.path.getsize(path) == 84 + 50 * n
    return n


def _small_torus(n, seed, centre=(0.0, 0.0, 0.0)):
    """A third of the unit torus: mesh_360's radius 0.1 is the unit torus's 0.3."""
    return oo.torus(n, seed, R=1.0 / 3.0, r=0.4 / 3.0, centre=centre)[0]


def _components(ms, mg, src, radius, max_nn, k):
    from structured_light_for_3d_model_replication_amd import ply
    P = ply.read_ply(src)[0]  # as the drop-in sees the points
    N = mg.estimate_normals(P, radius, max_nn)
    return ms.orient_normals_consistent_tangent_plane(P, N, k, radius=radius, info=True)[1]["components"]


def test_mesh_360_tangent_planes(ms, mg, pr, tmp_path, capsys):
    src, out = _write_ply(tmp_path / "torus.ply", _small_torus(2000, 4)), str(tmp_path / "torus.stl")
    assert _components(ms, mg, src, 0.1, 30, 12) == 1
    pr.ProcessingLogic.mesh_360(src, out, depth=5, density_trim=0.0, orientation_mode="tangent", tangent_planes=12)
    lines = capsys.readouterr().out.splitlines()
    assert lines == [f"[360 Mesh] Loading {src}...", "[360 Mesh] Estimating normals...",
                     "[360 Mesh] Re-orienting normals (Mode: tangent)...",
                     "[360 Mesh] Consistent tangent plane orientation applied.",
                     "[360 Mesh] Poisson Reconstruction (depth=5)...",
                     "[360 Mesh] Density trim is 0.0 -> Keeping watertight result.", f"[360 Mesh] Saved to {out}"]
    assert _stl_triangles(out) > 1000
    # "radial" ignores the argument
    rad, rad2 = str(tmp_path / "rad.stl"), str(tmp_path / "rad2.stl")
    pr.ProcessingLogic.mesh_360(src, rad, depth=5, orientation_mode="radial", tangent_planes=12)
    assert "[360 Mesh] Radial orientation applied (Outwards)." in capsys.readouterr().out
    pr.ProcessingLogic.mesh_360(src, rad2, depth=5, orientation_mode="radial")
    assert open(rad, "rb").read() == open(rad2, "rb").read()
    assert open(rad, "rb").read() != open(out, "rb").read()


def test_mesh_360_falls_back_on_a_disconnected_graph(ms, mg, pr, tmp_path, capsys):
    P = np.concatenate([_small_torus(1500, 5), _small_torus(1500, 6, centre=(5.0 / 3.0, 0.0, 0.0))])
    src, out = _write_ply(tmp_path / "two.ply", P), str(tmp_path / "two.stl")
    comps = _components(ms, mg, src, 0.1, 30, 12)
    assert comps == 2
    pr.ProcessingLogic.mesh_360(src, out, depth=5, tangent_planes=12)
    lines = capsys.readouterr().out.splitlines()
    assert lines[3] == f"[360 Mesh] Warning: Tangent plane failed (graph has {comps} components). Fallback to radial."
    assert lines[2] == "[360 Mesh] Re-orienting normals (Mode: tangent)..." and lines[-1] == f"[360 Mesh] Saved to {out}"
    ref = str(tmp_path / "ref.stl")
    pr.ProcessingLogic.mesh_360(src, ref, depth=5, orientation_mode="radial")
    assert open(ref, "rb").read() == open(out, "rb").read()  # the fall-back is the radial orientation


def test_reconstruct_stl_tangent_planes(pr, tmp_path, capsys):
    P, _ = oo.torus(3000, 9, centre=(0.0, 0.0, 5.0))
    src, out = _write_ply(tmp_path / "bare.ply", P), str(tmp_path / "bare.stl")
    pr.ProcessingLogic.reconstruct_stl(src, out, "watertight", {"depth": 5}, tangent_planes=12)
    lines = capsys.readouterr().out.splitlines()
    assert lines == [f"[Recon] Loading {src}...", "[Recon] Estimating normals...",
                     "[Recon] Poisson Reconstruction (depth=5)...", "[Recon] Computing normals and saving...",
                     f"[Recon] Saved STL to {out}"]
    assert _stl_triangles(out) > 0
    cam = str(tmp_path / "cam.stl")
    pr.ProcessingLogic.reconstruct_stl(src, cam, "watertight", {"depth": 5})
    assert open(cam, "rb").read() != open(out, "rb").read()


def test_tangent_planes_none_changes_nothing(pr, tmp_path, capsys):
    src = _write_ply(tmp_path / "torus.ply", _small_torus(2000, 4))
    names = [str(tmp_path / f"{i}.stl") for i in range(4)]
    L = pr.ProcessingLogic
    L.mesh_360(src, names[0], depth=5)
    a = capsys.readouterr().out
    L.mesh_360(src, names[1], depth=5, tangent_planes=None)
    b = capsys.readouterr().out
    assert a.replace(names[0], names[1]) == b and "Tangent plane failed (not provided)" in a
    L.reconstruct_stl(src, names[2], params={"depth": 5})
    a = capsys.readouterr().out
    L.reconstruct_stl(src, names[3], params={"depth": 5}, tangent_planes=None)
    b = capsys.readouterr().out
    assert a.replace(names[2], names[3]) == b
    assert open(names[0], "rb").read() == open(names[1], "rb").read()
    assert open(names[2], "rb").read() == open(names[3], "rb").read()
