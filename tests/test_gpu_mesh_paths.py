"""The Poisson meshing kernels (csrc/slmesh.inl, mesh.py) on the paths a cloud
inside its own bounding box never takes, against tests/mesh_oracle.py on the
inputs of tests/mesh_cases.py -- tests/test_mesh_oracle.py proves on the CPU
that each input reaches its path.  Everything but the FFT solve is compared
bit for bit; where the oracle's value is NaN, a NaN is required at the same
place (its sign and payload may differ between hosts).  The direct cases call
the C entry points with an explicit origin and h; the rest use mesh.py."""
import numpy as np
import pytest
import torch

from tests import mesh_cases as mc
from tests import mesh_oracle as mo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ms():
    from structured_light_for_3d_model_replication_amd import mesh
    return mesh


def _dev(ms, a, dtype=None):
    """A fresh device tensor of a (possibly read-only) array."""
    t = torch.from_numpy(np.array(a, dtype=dtype))
    return t.to(ms._engine(None).device).contiguous()


def _same_bits(got, exp):
    """Equal bit for bit, except that a NaN of the oracle only asks for a NaN."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape
    np.testing.assert_array_equal(got, exp)  # (NaN at the same places)
    ints = {4: np.uint32, 8: np.uint64}[exp.dtype.itemsize]
    there = ~np.isnan(exp) if exp.dtype.kind == "f" else np.ones(exp.shape, bool)
    np.testing.assert_array_equal(got.view(ints)[there], exp.view(ints)[there])


def _splat(ms, P, N, depth, origin=mc.ZERO3, h=1.0):
    """sl_mesh_splat and sl_mesh_unfix -> (sums int64 [4, R^3], grids f32 [4, R^3])."""
    eng = ms._engine(None)
    R = 1 << depth
    Pd, Nd = _dev(ms, P, np.float64), _dev(ms, N, np.float64)
    acc = torch.zeros((4, R * R * R), dtype=torch.int64, device=eng.device)
    ms._call(eng, "sl_mesh_splat", ms._ptr(Pd), ms._ptr(Nd), len(P), depth, ms._origin(origin), float(h),
             ms._ptr(acc))
    G = torch.empty((4, R * R * R), dtype=torch.float32, device=eng.device)
    ms._call(eng, "sl_mesh_unfix", ms._ptr(acc), acc.numel(), ms._ptr(G))
    return acc.cpu().numpy(), G.cpu().numpy()


# ---- gaps 1-4: fix()'s rounding and saturation, the wrapping sums, corners() outside the box ---------------
@pytest.mark.parametrize("name", mc.SPLAT_CASES)
def test_splat_cases(ms, name):
    P, N, depth = mc.splat_case(name)
    acc, G = _splat(ms, P, N, depth)
    exp = mo.splat_sums(P, N, mc.ZERO3, 1.0, 1 << depth)
    np.testing.assert_array_equal(acc, exp)
    _same_bits(G, mo.unfix(exp))
    acc2, G2 = _splat(ms, P, N, depth)
    np.testing.assert_array_equal(acc2, acc)
    np.testing.assert_array_equal(G2.view(np.uint32), G.view(np.uint32))
    if name == "wrap":
        node = (3 * 4 + 1) * 4 + 2
        assert G[1, node] == -2.0 ** 33 == G[2, node] and G[0, node] == 4.0
    if name == "saturate":
        assert G[0].sum() == 18.0 and np.isfinite(G).all() and G.max() == np.float32(2.0 ** 32)


@pytest.mark.parametrize("depth", [1, 3])
def test_sample_outside_the_box(ms, depth):
    R = 1 << depth
    G = np.random.default_rng(50 + depth).normal(size=(R, R, R)).astype(np.float32)
    P = mc.outside_points(R)
    got = ms.sample(_dev(ms, G), _dev(ms, P), mc.ZERO3, 1.0).cpu().numpy()
    exp = mo.sample(G, P, mc.ZERO3, 1.0)
    assert np.isnan(exp).sum() == (~np.isfinite(P)).any(1).sum() > 0
    _same_bits(got, exp)


# ---- gap 5: grids smaller than a workgroup -------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("kind", mc.CLOUD_KINDS)
def test_small_grid_chain(ms, kind, depth):
    """8 and 64 nodes against 256 threads: every stage on the GPU's own output of the stage before it."""
    R = 1 << depth
    P, N, scale = mc.cloud(kind, 257, R, seed=258 + depth)
    f = ms.poisson_field(P, N, depth, scale, keep=True)
    o, h, _ = mo.box(P, depth, scale)
    W, V = mo.splat(P, N, o, h, R)
    _same_bits(f["W"].cpu().numpy(), W)
    _same_bits(f["V"].cpu().numpy(), V)
    div = f["div"].cpu().numpy()
    _same_bits(div, mo.divergence(V, h))
    if depth == 1:  # the +-1 neighbours are the same node
        assert not div.any() and not np.signbit(div).any()
    chi = f["chi"].cpu().numpy()
    assert chi.shape == (R, R, R) and np.isfinite(chi).all()
    assert f["iso"] == mo.iso_value(chi, P, o, h)
    Vg, Tg = ms.extract_isosurface(f["chi"], f["iso"], f["origin"], f["h"])
    Vo, To = mo.extract(chi, f["iso"], o, h)
    np.testing.assert_array_equal(Tg.cpu().numpy(), To)
    _same_bits(Vg.cpu().numpy(), Vo)
    if len(Vo):
        _same_bits(ms.vertex_density(f["W"], Vg, f["origin"], f["h"]).cpu().numpy(), mo.sample(W, Vo, o, h))


# ---- gaps 5-7: extraction at R = 2 and 4, all 84 (tetrahedron, case) pairs, closedness, special values -------
@pytest.mark.parametrize("name", [n for n in mc.fields() if n != "constant"])
def test_extraction_fields(ms, name):
    chi, iso = mc.fields()[name]
    o, h = (mc.ZERO3, 1.0) if name in mc.SPECIAL else (mc.SEAM_ORIGIN, mc.SEAM_H)
    V, T = ms.extract_isosurface(_dev(ms, chi), iso, o, h)
    V2, T2 = ms.extract_isosurface(_dev(ms, chi), iso, o, h)
    Vo, To = mo.extract(chi, iso, o, h)
    V, T = V.cpu().numpy(), T.cpu().numpy()
    assert T.dtype == np.int32 and len(To) > 0
    np.testing.assert_array_equal(T, To)
    _same_bits(V, Vo)
    np.testing.assert_array_equal(T2.cpu().numpy(), T)
    np.testing.assert_array_equal(V2.cpu().numpy().view(np.uint64), V.view(np.uint64))
    if name in mc.ALL_PAIRS:
        assert len(mo.tet_pairs(chi, iso)) == 84
    if name in mc.CLOSED:
        assert mo.edge_census(T)[0]


@pytest.mark.parametrize("name", list(mc.divergence_fields()))
def test_divergence_special_values(ms, name):
    V, h = mc.divergence_fields()[name]
    eng = ms._engine(None)
    Vd = _dev(ms, V)
    div = torch.empty((4, 4, 4), dtype=torch.float32, device=eng.device)
    ms._call(eng, "sl_mesh_divergence", ms._ptr(Vd), 2, float(h), ms._ptr(div))
    exp = mo.divergence(V, h)
    assert (exp != 0).sum() > 32
    _same_bits(div.cpu().numpy(), exp)


@pytest.mark.parametrize("name", mc.SPECIAL)
def test_sample_special_fields(ms, name):
    G, _ = mc.fields()[name]
    rng = np.random.default_rng(9)
    P = np.concatenate([rng.random((300, 3)) * 12.0 - 4.0, rng.integers(-2, 7, size=(60, 3)).astype(np.float64)])
    got = ms.sample(_dev(ms, G), _dev(ms, P), mc.ZERO3, 1.0).cpu().numpy()
    exp = mo.sample(G, P, mc.ZERO3, 1.0)
    assert (exp != 0).sum() > 100
    _same_bits(got, exp)


# ---- gap 8: sampling across the seam -------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["seam", "random"])
def test_sample_at_the_seam_fields_vertices(ms, grid):
    G, _ = mc.fields()[grid]
    P = mc.seam_vertices()
    got = ms.sample(_dev(ms, G), _dev(ms, P), mc.SEAM_ORIGIN, mc.SEAM_H).cpu().numpy()
    _same_bits(got, mo.sample(G, P, mc.SEAM_ORIGIN, mc.SEAM_H))
    # the extraction's own vertices of the field: the same bits as the oracle's, so the same samples
    chi, iso = mc.fields()["seam"]
    V, _ = ms.extract_isosurface(_dev(ms, chi), iso, mc.SEAM_ORIGIN, mc.SEAM_H)
    d = ms.vertex_density(_dev(ms, G), V, mc.SEAM_ORIGIN, mc.SEAM_H).cpu().numpy()
    np.testing.assert_array_equal(d.view(np.uint64), got.view(np.uint64))


def test_sample_is_periodic(ms):
    G, _ = mc.fields()["random"]
    p, shifted = mc.periodic_points()
    Gd = _dev(ms, G)
    got = ms.sample(Gd, _dev(ms, p), mc.PERIODIC_ORIGIN, mc.PERIODIC_H).cpu().numpy()
    _same_bits(got, mo.sample(G, p, mc.PERIODIC_ORIGIN, mc.PERIODIC_H))
    for q in shifted:
        again = ms.sample(Gd, _dev(ms, q), mc.PERIODIC_ORIGIN, mc.PERIODIC_H).cpu().numpy()
        np.testing.assert_array_equal(again.view(np.uint64), got.view(np.uint64))


# ---- gap 9: sl_mesh_remove_vertices ---------------------------------------------------------------------------
@pytest.mark.parametrize("nt", mc.TRIM_COUNTS)
@pytest.mark.parametrize("nv", mc.TRIM_COUNTS)
def test_remove_vertices(ms, nv, nt):
    for mask in mc.TRIM_MASKS:
        V, T, m = mc.trim_case(nv, nt, mask)
        V2, T2 = ms.remove_vertices_by_mask(_dev(ms, V), _dev(ms, T), _dev(ms, m))
        Vo, To = mo.remove_vertices_by_mask(V, T, m)
        assert V2.dtype == torch.float64 and T2.dtype == torch.int32
        assert tuple(V2.shape) == Vo.shape and tuple(T2.shape) == To.shape, mask
        np.testing.assert_array_equal(V2.cpu().numpy().view(np.uint64), Vo.view(np.uint64))
        np.testing.assert_array_equal(T2.cpu().numpy(), To)


# ---- gap 10: sl_ordered_sum ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", mc.OSUM_N)
def test_ordered_sum(ms, n):
    whole = _dev(ms, mc.osum_values(n))
    for stride, offset in mc.OSUM_STRIDES:
        flat, v = mc.osum_case(n, stride, offset)
        got = ms.ordered_sum(whole[: stride * n], stride, offset)
        assert got == mo.ordered_sum(v), (stride, offset)


# ---- gap 11: k_orient -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", mc.ORIENT_N)
def test_orient_towards_location(ms, n):
    P, N, loc, rows = mc.orient_case(n)
    got = ms.orient_normals_towards_camera_location(_dev(ms, P), _dev(ms, N), loc).cpu().numpy()
    np.testing.assert_array_equal(got.view(np.uint64), mo.orient_towards(P, N, loc).view(np.uint64))
    for key in ("dot_plus_zero", "dot_minus_zero", "last_plus_zero"):  # n . (loc - p) == 0: kept
        np.testing.assert_array_equal(got[rows[key]].view(np.uint64), N[rows[key]].view(np.uint64))
    np.testing.assert_array_equal(got[rows["at_location"]], [0.0, 0.0, 1.0])
    assert got[rows["negative_zero_normal"]].tolist() == (np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)).tolist()


# ---- gap 12: mesh.solve at R = 2, 4, 8 and on a divergence of non-zero mean -------------------------------------
@pytest.mark.parametrize("depth,seed,shift", mc.SOLVE_CASES)
def test_solve_small_grids(ms, depth, seed, shift):
    """max |chi - f64 solve| / max |f64 solve| <= 8 x the same error of mesh.solve on CPU tensors (torch's CPU
    f32 FFT) for this very input: test_gpu_mesh.test_solve's margin, which covers rocFFT's other butterfly
    order.  With a non-zero mean of the divergence, chi^(0) = 0 keeps the mean of chi within the same bound."""
    div = mc.solve_case(depth, seed, shift)
    ref = mo.solve(div, mc.SOLVE_H)
    top = np.abs(ref).max()
    cpu = ms.solve(torch.from_numpy(div.copy()), mc.SOLVE_H).numpy()
    bound = 8.0 * np.abs(cpu - ref).max() / top
    chi = ms.solve(_dev(ms, div), mc.SOLVE_H)
    assert chi.dtype == torch.float32 and chi.is_contiguous() and tuple(chi.shape) == div.shape
    chi = chi.cpu().numpy()
    err = np.abs(chi - ref).max() / top
    mean = abs(float(chi.mean(dtype=np.float64))) / top
    print(f"R = {1 << depth} seed {seed} shift {shift}: relative error {err:.3e}, mean {mean:.3e}, bound {bound:.3e}")
    assert 0.0 < bound < 1e-5
    assert err <= bound
    if shift:
        assert mean <= bound
