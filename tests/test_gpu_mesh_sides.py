"""The four features that start from the sorted side table (csrc/slprim.inl: sort_sides, run_sides) on the same tiny
meshes (tests/mesh_sides_cases.py): the components, the adjacency and one smoothing step, the checks and the hole
filling, each equal to its own CPU oracle exactly, and the three counts of the sides of multiplicity 1 equal to each
other."""
import numpy as np
import pytest

from tests import mesh_sides_cases as sc

pytestmark = pytest.mark.gpu

CASES = sc.cases()


@pytest.fixture(scope="module")
def ms():
    from structured_light_for_3d_model_replication_amd import mesh
    return mesh


def _np(x):
    return x.cpu().numpy()


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        g = _np(g)
        assert g.dtype == w.dtype and g.shape == w.shape
        np.testing.assert_array_equal(g, w)


def _same_dict(got, want):
    assert got == want
    assert {k: type(v) for k, v in got.items()} == {k: type(v) for k, v in want.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_consumer_equals_its_oracle(ms, name):
    T, nv = CASES[name]
    P = sc.vertices(nv)
    want = sc.reference(name)
    # the components (slmeshclean.inl)
    _same(ms.cluster_connected_triangles(P, T), want["cluster"])
    _same(ms.cluster_connected_triangles(None, T, n_vertices=nv)[:2], want["cluster"][:2])
    # the adjacency and a step on it (slmeshsmooth.inl)
    adjacency = ms.adjacency_list(T, nv, boundary=True)
    _same(adjacency, want["adjacency"])
    _same((ms.filter_smooth_taubin(P, T, iterations=1),), (want["taubin"],))
    # the checks (slmeshcheck.inl)
    check = ms.check(P, T)
    _same_dict(check, want["check"])
    for allow, edges in zip((True, False), want["edges"]):
        _same((ms.get_non_manifold_edges(None, T, allow, n_vertices=nv),), (edges,))
    _same((ms.get_non_manifold_vertices(None, T, n_vertices=nv),), (want["vertices"],))
    oriented, orientable = ms.orient_triangles(None, T, n_vertices=nv)
    _same((oriented,), (want["orient"][0],))
    assert orientable is want["orient"][1]
    # the hole filling (slmeshfill.inl)
    V, To, counts = ms.fill_holes(P, T, info=True)
    _same((V, To), want["fill"][:2])
    _same_dict(counts, want["fill"][2])
    loops = ms.boundary_loops(P, T)
    assert sorted(loops) == sorted(want["loops"])
    _same(tuple(loops[k] for k in sorted(loops)), tuple(want["loops"][k] for k in sorted(loops)))
    # one table, one count of the sides of multiplicity 1
    open_sides, self_loops = sc.EXPECTED[name]
    assert check["boundary_edges"] == counts["boundary_sides"] == open_sides + self_loops
    assert int(_np(loops["size"]).sum()) == counts["boundary_sides"]
