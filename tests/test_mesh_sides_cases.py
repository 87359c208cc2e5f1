"""The side-table cases (tests/mesh_sides_cases.py) on the CPU: the four features' oracles agree on how many sides
have multiplicity 1, and on what was worked out by hand, before a device is asked."""
import numpy as np
import pytest

from tests import mesh_sides_cases as sc

CASES = sc.cases()


def test_the_cases_are_the_listed_ones():
    assert sorted(CASES) == sorted(sc.EXPECTED)
    for T, nv in CASES.values():
        assert T.dtype == np.int32 and T.ndim == 2 and T.shape[1] == 3 and 0 <= T.min() and T.max() < nv
    T, nv = CASES["capped_strip_unreferenced"]
    assert T.max() == nv - 2                                    # V exceeds the largest index
    T, nv = CASES["fan_over_tile"]
    assert sc.RADIX_TILE < 3 * len(T) <= sc.RADIX_TILE + 3      # just over one tile of the sort


def test_a_run_straddles_the_tile_edge():
    T, nv = CASES["fan_over_tile"]
    keys = np.sort(sc.ko.sides(T, nv)[0].reshape(-1))
    assert keys[sc.RADIX_TILE - 1] == keys[sc.RADIX_TILE]
    assert keys[sc.RADIX_TILE - 2] != keys[sc.RADIX_TILE - 1] and keys[sc.RADIX_TILE] != keys[sc.RADIX_TILE + 1]


@pytest.mark.parametrize("name", sorted(CASES))
def test_boundary_counts_agree(name):
    T, nv = CASES[name]
    check, fill, open_sides, loops = sc.boundary_counts(T, nv)
    assert (open_sides, loops) == sc.EXPECTED[name]
    assert check == fill == open_sides + loops
    ref = sc.reference(name)
    assert ref["check"]["boundary_edges"] == check and ref["fill"][2]["boundary_sides"] == fill
    assert int(ref["loops"]["size"].sum()) == fill
    ends = {v for (v, w), n in sc.so._sets(T, nv)[1].items() if v != w and n == 1}
    assert set(np.nonzero(ref["adjacency"][2])[0].tolist()) == ends        # the boundary flags are those sides' ends


def test_what_the_cases_are_for():
    c = sc.reference("all_zero")["check"]
    assert c["edges"] == 1 and c["non_manifold_edges"] == 1 and c["degenerate_triangles"] == 1
    c = sc.reference("book_3_degenerate")["check"]
    assert c["non_manifold_edges"] == 1 and c["degenerate_triangles"] == 1 and not c["orientable"]
    c = sc.reference("two_tetrahedra_one_vertex")["check"]
    assert c["edge_manifold_closed"] and c["consistent"] and not c["vertex_manifold"]
    assert sc.reference("two_tetrahedra_one_vertex")["vertices"].tolist() == [0]
    assert sc.reference("two_tetrahedra_one_vertex")["cluster"][1].tolist() == [4, 4]
    c = sc.reference("duplicated_triangle")["check"]
    assert c["edges"] == 3 and c["inconsistent_edges"] == 3 and c["boundary_edges"] == 0
    V, T, counts = sc.reference("capped_strip_unreferenced")["fill"]
    assert counts["filled"] == 1 and counts["new_vertices"] == 1 and counts["new_triangles"] == 4
    assert sc.ko.check(V, T)["boundary_edges"] == 0 and len(V) == 10
    assert sc.reference("fan_over_tile")["loops"]["size"].tolist() == [sc.RADIX_TILE // 3 + 3]
