"""The CPU restatement of the mesh smoothing (tests/meshsmooth_oracle.py) against itself: the order-free form the
device mirrors equals Open3D's loops taken literally on every case, the fold order shows in the bits, and ten
Taubin iterations do to a noisy sphere what the filter is for."""
import numpy as np
import pytest

from tests import meshsmooth_cases as cs
from tests import meshsmooth_oracle as so

ADJACENCY = cs.adjacency_cases()


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("name", sorted(ADJACENCY))
def test_adjacency_forms_agree(name):
    T, nv = ADJACENCY[name]
    got = so.adjacency_list(T, nv, boundary=True)
    _same(got, so.adjacency_list_sets(T, nv, boundary=True))
    _same(so.adjacency_list(T, nv), got[:2])
    rows, nb, bnd = got
    assert rows.dtype == np.int64 and nb.dtype == np.int32 and bnd.dtype == bool
    assert rows.shape == (nv + 1,) and rows[0] == 0 and rows[-1] == len(nb) and (np.diff(rows) >= 0).all()
    for v in np.nonzero(np.diff(rows))[0][:300]:
        assert (np.diff(nb[rows[v]:rows[v + 1]]) > 0).all()       # ascending, no duplicates


def test_adjacency_by_hand():
    rows, nb, bnd = so.adjacency_list(*ADJACENCY["aab"], boundary=True)
    assert rows.tolist() == [0, 2, 3] and nb.tolist() == [0, 1, 0]          # N(0) = {0, 1}
    assert bnd.tolist() == [False, False]                                  # {0, 1} is a side twice
    rows, nb, bnd = so.adjacency_list(*ADJACENCY["aaa"], boundary=True)
    assert rows.tolist() == [0, 0, 0, 1, 1] and nb.tolist() == [2] and not bnd.any()
    rows, nb, bnd = so.adjacency_list(*ADJACENCY["shared_edge"], boundary=True)
    assert rows.tolist() == [0, 2, 5, 8, 10] and nb.tolist() == [1, 2, 0, 2, 3, 0, 1, 3, 1, 2]
    assert bnd.all()
    rows, nb, bnd = so.adjacency_list(*ADJACENCY["empty_first_and_last_rows"], boundary=True)
    assert rows[0] == rows[1] == 0 and rows[-1] == rows[-2] and rows[5] == rows[6]
    rows, nb, bnd = so.adjacency_list(*ADJACENCY["sphere"], boundary=True)
    assert not bnd.any() and np.diff(rows).tolist() == [24] + [5] * 24 + [6] * 312 + [5] * 24 + [24]
    rows, nb, bnd = so.adjacency_list(*ADJACENCY["sheet_9x7"], boundary=True)
    assert int(bnd.sum()) == 2 * (9 + 7) - 4
    for d in cs.HUB_DEGREES:
        T, nv, hub = cs.hub_fan(d, d)
        rows = so.adjacency_list(T, nv)[0]
        assert rows[hub + 1] - rows[hub] == d


@pytest.mark.parametrize("name", sorted(cs.BAD_INDEX_CASES))
def test_bad_indices_raise(name):
    T, nv = cs.BAD_INDEX_CASES[name]
    for fn in (so.adjacency_list, so.adjacency_list_sets):
        with pytest.raises(IndexError, match="triangle index out of range"):
            fn(T, nv)
    for fn in list(so.FILTERS.values()) + list(so.FILTERS_SETS.values()):
        with pytest.raises(IndexError, match="triangle index out of range"):
            fn(np.zeros((nv, 3)), T)


@pytest.mark.parametrize("run", sorted(cs.RUNS))
def test_filter_forms_agree(run):
    mesh, method, kw = cs.RUNS[run]
    P, T = cs.MESHES[mesh]
    before = P.copy()
    want = so.FILTERS_SETS[method](P, T, **kw)
    got = cs.reference(run)
    assert got.dtype == np.float64 and got.shape == P.shape and np.isfinite(got).all()
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(P, before)
    if kw.get("iterations", 1) == 0:
        np.testing.assert_array_equal(got, P)


def test_argument_errors():
    P, T = cs.MESHES["coincident"]
    bad = P.copy()
    bad[2, 1] = np.inf
    for forms in (so.FILTERS, so.FILTERS_SETS):
        for fn in forms.values():
            with pytest.raises(ValueError):
                fn(P, T, -1)
            with pytest.raises(ValueError, match="non-finite"):
                fn(bad, T)
        for v in (np.nan, np.inf):
            with pytest.raises(ValueError):
                forms["laplacian"](P, T, 1, v)
            with pytest.raises(ValueError):
                forms["taubin"](P, T, 1, v)
            with pytest.raises(ValueError):
                forms["taubin"](P, T, 1, 0.5, v)


def test_the_fold_order_is_part_of_the_result():
    """The spoke fan's hub row has weights over twelve decades: folded from its last entry to its first, the hub
    comes out with different bits (and the same value to rounding)."""
    P, T, hub = cs.spoke_fan()
    up = so.filter_smooth_laplacian(P, T, 1, 0.5)
    down = so.filter_smooth_laplacian(P, T, 1, 0.5, descending=True)
    assert (up[hub] != down[hub]).any()
    np.testing.assert_allclose(up, down, rtol=1e-9, atol=1e-9)


def test_fixed_boundary_and_empty_rows():
    P, T = cs.MESHES["isolated_and_unreferenced"]
    for method in ("laplacian", "taubin"):
        out = so.FILTERS[method](P, T, 3)
        np.testing.assert_array_equal(out[[0, 7]], P[[0, 7]])      # an empty row keeps its vertex
        np.testing.assert_array_equal(out[6], P[6])                # N(6) = {6}: the mean of itself
        assert (out[1:6] != P[1:6]).any(axis=1).all()
    np.testing.assert_array_equal(so.filter_smooth_simple(P, T, 3)[[0, 7]], P[[0, 7]])
    P, T = cs.MESHES["strip_257"]
    np.testing.assert_array_equal(cs.reference("strip_257-taubin-iterations=2-fixed_boundary=True"), P)
    P, T = cs.MESHES["sheet_9x7"]
    bnd = so.adjacency_list(T, len(P), boundary=True)[2]
    out = cs.reference("sheet_9x7-laplacian-iterations=2-fixed_boundary=True")
    np.testing.assert_array_equal(out[bnd], P[bnd])
    assert (out[~bnd] != P[~bnd]).any(axis=1).all()
    for method in ("simple", "laplacian", "taubin"):                # a closed mesh: nothing is fixed
        np.testing.assert_array_equal(cs.reference(f"noisy_sphere-{method}-iterations=2-fixed_boundary=True"),
                                      cs.reference(f"noisy_sphere-{method}-iterations=2"))


def test_taubin_smooths_without_shrinking():
    """The noisy sphere (radial std 0.0182, mean radius 0.998): ten Taubin iterations leave std 0.0061 and mean
    radius 1.003; ten Laplacian iterations shrink it to mean radius 0.897."""
    P, T = cs.noisy_sphere()
    r0 = np.linalg.norm(P, axis=1)
    rt = np.linalg.norm(cs.reference("noisy_sphere-taubin-iterations=10"), axis=1)
    rl = np.linalg.norm(cs.reference("noisy_sphere-laplacian-iterations=10"), axis=1)
    print(f"input std {r0.std():.4f} mean {r0.mean():.4f}; taubin std {rt.std():.4f} mean {rt.mean():.4f}; "
          f"laplacian mean {rl.mean():.4f}")
    assert rt.std() <= 0.5 * r0.std()
    assert abs(rt.mean() - r0.mean()) <= 0.01
    assert rl.mean() < 0.95
