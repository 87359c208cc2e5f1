"""The mesh checks' CPU restatement (tests/meshcheck_oracle.py) against itself: the order-free forms the kernels compute
equal the sequential Open3D-style loops, the known answers come out exactly, and nothing depends on the numbering."""
import numpy as np
import pytest

from tests import meshcheck_cases as kc
from tests import meshcheck_oracle as ko
from tests import meshclean_cases as mc
from tests import meshclean_oracle as mco

CASES = kc.cases()
COUNTS = ("vertices", "triangles", "edges", "boundary_edges", "non_manifold_edges", "inconsistent_edges",
          "non_manifold_vertices", "degenerate_triangles", "edge_manifold", "edge_manifold_closed", "vertex_manifold",
          "orientable", "consistent", "watertight")


def _random_meshes(count, degenerate, seed):
    """Meshes of up to 8 vertices and 11 triangles; ``degenerate``: indices may repeat within a triangle."""
    rng = np.random.default_rng(seed)
    for _ in range(count):
        nv, nt = int(rng.integers(3, 9)), int(rng.integers(1, 12))
        if degenerate:
            T = rng.integers(0, nv, size=(nt, 3))
        else:
            T = np.stack([rng.permutation(nv)[:3] for _ in range(nt)])
        yield T.astype(np.int32), nv


@pytest.mark.parametrize("name", sorted(CASES))
def test_orientation_equals_the_sequential_loop(name):
    _, T, nv = CASES[name]
    got, ok = kc.reference(name, "orient")
    want, want_ok = ko.orient_triangles_sequential(T, nv)
    assert ok == want_ok
    np.testing.assert_array_equal(got, want)
    assert got.dtype == np.int32 and got.shape == T.shape
    if ok:
        assert ko.edge_counts(got, nv)["inconsistent_edges"] == 0
    else:
        np.testing.assert_array_equal(got, T)


@pytest.mark.parametrize("degenerate", [False, True])
def test_orientation_equals_the_sequential_loop_on_random_meshes(degenerate):
    seen = set()
    for T, nv in _random_meshes(3000, degenerate, 5 + degenerate):
        got, ok = ko.orient_triangles(T, nv)
        want, want_ok = ko.orient_triangles_sequential(T, nv)
        assert ok == want_ok, T
        np.testing.assert_array_equal(got, want)
        seen.add(ok)
    assert seen == {False, True}


@pytest.mark.parametrize("name", sorted(n for n, (_, T, _) in CASES.items() if not ko.degenerate(T).any()))
def test_vertex_test_equals_the_link_search(name):
    _, T, nv = CASES[name]
    got = kc.reference(name, "vertices")
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, ko.get_non_manifold_vertices_link(T, nv))


def test_vertex_test_equals_the_link_search_on_random_meshes():
    hits = 0
    for T, nv in _random_meshes(3000, False, 11):
        got = ko.get_non_manifold_vertices(T, nv)
        np.testing.assert_array_equal(got, ko.get_non_manifold_vertices_link(T, nv))
        hits += len(got) > 0
    assert 0 < hits < 3000


def test_degenerate_triangles_take_no_part_in_the_vertex_test():
    _, T, nv = CASES["degenerate_in_run"]
    np.testing.assert_array_equal(ko.get_non_manifold_vertices(T, nv),
                                  ko.get_non_manifold_vertices(ko.remove_degenerate_triangles(T, nv), nv))
    with pytest.raises(ValueError):
        ko.get_non_manifold_vertices_link(T, nv)


def test_known_answers():
    c = kc.reference("tetrahedron", "check")
    assert c["watertight"] and c["orientable"] and c["signed_volume"] == 1.0 / 6.0
    c = kc.reference("cube", "check")
    assert c["watertight"] and c["triangles"] == 12 and c["edges"] == 18 and c["area"] == 6.0
    assert c["volume"] == 1.0 and c["signed_volume"] == 1.0
    for name in kc.closed_meshes():
        c, f, h = (kc.reference(name + tag, "check") for tag in ("", "_all_flipped", "_half_flipped"))
        assert c["watertight"] and c["signed_volume"] > 0.0
        assert f["watertight"] and f["signed_volume"] == -c["signed_volume"] and f["area"] == c["area"]
        assert h["edge_manifold_closed"] and h["vertex_manifold"] and h["orientable"] and not h["consistent"]
        assert not h["watertight"] and h["volume"] is None
    s = kc.reference("sphere", "check")
    assert abs(s["volume"] - 4.0 * np.pi / 3.0) < 0.1 and abs(s["area"] - 4.0 * np.pi) < 0.2   # inscribed: below
    for n in kc.MOBIUS_QUADS:
        c = kc.reference(f"mobius_{n}", "check")
        assert c["edge_manifold"] and c["vertex_manifold"] and not c["orientable"] and c["boundary_edges"] == 2 * n
    c = kc.reference("klein_8x9", "check")
    assert c["edge_manifold_closed"] and c["vertex_manifold"] and not c["orientable"] and not c["consistent"]
    assert not c["watertight"] and c["volume"] is None
    with pytest.raises(ValueError, match="not watertight"):
        ko.get_volume(*CASES["klein_8x9"][:2])
    for m in kc.BOOK_PAGES:
        c = kc.reference(f"book_{m}", "check")
        assert c["non_manifold_edges"] == 1 and c["boundary_edges"] == 2 * m and not c["orientable"]
        np.testing.assert_array_equal(kc.reference(f"book_{m}", "edges"), [[0, 1]])
        assert len(kc.reference(f"book_{m}", "edges_closed")) == 2 * m + 1
    for d in (63, 4097):
        assert kc.reference(f"fan_{d}", "check")["vertex_manifold"]
        assert kc.reference(f"cone_{d}", "check")["vertex_manifold"]
    np.testing.assert_array_equal(kc.reference("two_tetrahedra_one_vertex", "vertices"), [0])
    assert kc.reference("two_tetrahedra_one_vertex", "check")["edge_manifold_closed"]
    assert len(kc.reference("two_cones_one_apex", "vertices")) == 1
    np.testing.assert_array_equal(kc.reference("fans_65_at_hub", "vertices"), [0])
    c = kc.reference("two_tetrahedra_one_edge", "check")
    assert c["non_manifold_edges"] == 1 and not c["orientable"]
    c = kc.reference("aab", "check")      # (0, 0, 1): {0, 0} once, {0, 1} twice
    assert (c["edges"], c["boundary_edges"], c["degenerate_triangles"], c["inconsistent_edges"]) == (2, 1, 1, 0)
    c = kc.reference("aaa", "check")
    assert (c["edges"], c["non_manifold_edges"], c["orientable"]) == (1, 1, False)
    c = kc.reference("same_twice", "check")
    assert c["inconsistent_edges"] == 3 and c["orientable"]
    for name in ("none", "nothing"):
        c = kc.reference(name, "check")
        assert c["watertight"] and c["orientable"] and c["edges"] == 0


@pytest.mark.parametrize("name", kc.STRUCTURED_SHUFFLED)
def test_numbering_does_not_matter(name):
    a, b = kc.reference(name, "check"), kc.reference(name + "_shuffled", "check")
    assert {k: a[k] for k in COUNTS} == {k: b[k] for k in COUNTS}
    assert len(kc.reference(name, "edges_closed")) == len(kc.reference(name + "_shuffled", "edges_closed"))
    if a["area"] is not None:        # the sums run in another order: the last bits may differ
        assert b["area"] == pytest.approx(a["area"], rel=1e-12)
        if a["watertight"]:
            assert b["signed_volume"] == pytest.approx(a["signed_volume"], rel=1e-11)


@pytest.mark.parametrize("name", ["own_voxels", "live_4097"])
def test_remove_duplicated_is_the_tail_of_simplify(name):
    """Every vertex alone in its voxel: simplify_loop maps nothing, and what it then does to the triangles is
    remove_degenerate + remove_duplicated, stored rotated."""
    P, T, vs = mc.simplify_cases()[name]
    Vs, Ts = mco.simplify_loop(P, T, vs)
    np.testing.assert_array_equal(Vs, P)
    kept = ko.remove_duplicated_triangles(ko.remove_degenerate_triangles(T, len(P)), len(P))
    assert 0 < len(kept) < len(T)
    np.testing.assert_array_equal(np.array([mco._rotate(tuple(t)) for t in kept], dtype=np.int32), Ts)


@pytest.mark.parametrize("name", ["repeats_mixed", "same_twice", "opposite_windings", "aaa", "none", "v_17"])
def test_removals(name):
    _, T, nv = CASES[name]
    kept = kc.reference(name, "degenerate")
    assert kept.dtype == np.int32 and len(kept) == len(T) - kc.reference(name, "check")["degenerate_triangles"]
    dup = kc.reference(name, "duplicated")
    assert dup.dtype == np.int32 and dup.shape[1:] == (3,)
    assert len({mco._rotate(tuple(int(x) for x in t)) for t in T}) == len(dup)
    if name == "same_twice":
        np.testing.assert_array_equal(dup, T[:1])
    if name == "opposite_windings":
        np.testing.assert_array_equal(dup, T)


def test_bad_indices_raise():
    for T, nv in kc.BAD_INDEX_CASES.values():
        for fn in (ko.edge_counts, ko.get_non_manifold_edges, ko.get_non_manifold_vertices, ko.orient_triangles,
                   ko.remove_degenerate_triangles, ko.remove_duplicated_triangles):
            with pytest.raises(IndexError, match="triangle index out of range"):
                fn(T, nv)
