"""The CPU restatement of the mesh clean-up (tests/meshclean_oracle.py): its order-free forms equal the
sequential loops they restate, and every named case meets the precondition it is named for."""
import numpy as np
import pytest

from tests import mesh_oracle as mo
from tests import meshclean_cases as cs
from tests import meshclean_oracle as oc

COMPONENTS = cs.components_cases()
SIMPLIFY = cs.simplify_cases()


@pytest.mark.parametrize("name", sorted(COMPONENTS))
def test_labels_equal_the_breadth_first_loop(name):
    T, nv = COMPONENTS[name]
    labels, counts, area = oc.cluster_connected_triangles(T, nv)
    seq_labels, seq_counts = oc.cluster_sequential(T, nv)
    np.testing.assert_array_equal(labels, seq_labels)
    np.testing.assert_array_equal(counts, seq_counts)
    assert area is None and labels.dtype == np.int32 and counts.dtype == np.int64
    assert counts.sum() == len(T) and (len(T) == 0 or labels.max() == len(counts) - 1)


def test_labels_equal_scipy_components():
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    for name, (T, nv) in COMPONENTS.items():
        if len(T) == 0:
            continue
        keys = oc.edge_keys(T, nv).reshape(-1)
        vals = np.repeat(np.arange(len(T)), 3)
        order = np.argsort(keys, kind="stable")
        keys, vals = keys[order], vals[order]
        same = np.nonzero(keys[1:] == keys[:-1])[0] + 1
        g = sp.coo_matrix((np.ones(len(same)), (vals[same], vals[same - 1])), shape=(len(T), len(T)))
        n, lab = connected_components(g, directed=False)
        labels, counts, _ = oc.cluster_connected_triangles(T, nv)
        assert n == len(counts), name
        _, first = np.unique(lab, return_index=True)            # relabel by smallest member
        relabel = np.empty(n, dtype=np.int64)
        relabel[np.argsort(first)] = np.arange(n)
        np.testing.assert_array_equal(relabel[lab], labels, err_msg=name)


def test_components_preconditions():
    c = COMPONENTS
    assert oc.cluster_connected_triangles(*c["shared_edge"])[1].tolist() == [2]
    assert oc.cluster_connected_triangles(*c["shared_vertex_only"])[1].tolist() == [1, 1]
    assert oc.cluster_connected_triangles(*c["edge_of_3"])[1].tolist() == [3]
    assert oc.cluster_connected_triangles(*c["edge_of_5"])[0].tolist() == [0, 1, 0, 0, 0, 0]
    assert oc.cluster_connected_triangles(*c["same_twice"])[0].tolist() == [0, 1, 0]
    assert oc.cluster_connected_triangles(*c["opposite_windings"])[0].tolist() == [0, 1, 0]
    assert oc.cluster_connected_triangles(*c["degenerate_aab"])[0].tolist() == [0, 0, 1, 2, 2, 3]
    labels, counts, _ = oc.cluster_connected_triangles(*c["interleaved"])
    assert labels.tolist() == [0, 1, 2, 0, 1, 0]
    # ranking the roots by their position in edge-key order would label the cluster of triangle 1 first
    T, nv = c["interleaved"]
    assert oc.edge_keys(T, nv)[1].min() < oc.edge_keys(T, nv)[0].min()
    for n in (255, 256, 257, 4095, 4096, 4097):
        T, nv = c[f"strip_{n}"]
        assert len(T) == n and oc.cluster_connected_triangles(T, nv)[1].tolist() == [n]
        assert (np.diff(T[:, 0]) < 0).any()     # the numbering is shuffled
    assert oc.cluster_connected_triangles(*c["isolated_4097"])[1].tolist() == [1] * 4097
    bits = {v: int(v * v - 1).bit_length() for v in (15, 16, 17, 255, 256, 257, 65537)}
    assert [-(-bits[v] // 4) for v in (15, 16, 17, 255, 256, 257, 65537)] == [2, 2, 3, 4, 4, 5, 9]  # radix passes
    T, nv = c["v_2_31_minus_1"]
    assert nv == 2 ** 31 - 1 and int(oc.edge_keys(T, nv).max()).bit_length() == 62
    assert oc.cluster_connected_triangles(T, nv)[0].tolist() == [0, 1, 0, 1, 2, 0]
    for T, nv in c.values():
        assert T.dtype == np.int32 and (len(T) == 0 or (T.min() >= 0 and T.max() < nv))


@pytest.mark.parametrize("name", sorted(cs.BAD_INDEX_CASES))
def test_bad_indices_raise(name):
    T, nv = cs.BAD_INDEX_CASES[name]
    with pytest.raises(IndexError):
        oc.cluster_connected_triangles(T, nv)
    with pytest.raises(IndexError):
        oc.remove_unreferenced_vertices(np.zeros((nv, 3)), T)
    with pytest.raises(IndexError):
        oc.simplify_vertex_clustering(np.zeros((nv, 3)), T, 1.0)


def test_area_case():
    P, T, sizes = cs.area_case()
    labels, counts, area = oc.cluster_connected_triangles(T, len(P), P)
    assert counts.tolist() == sizes and sorted(sizes) == [1, 63, 64, 65, 129]
    np.testing.assert_array_equal(labels, oc.cluster_sequential(T, len(P))[0])
    A = oc.triangle_areas(P, T)
    assert (A == 0.0).sum() >= 8 and A.max() / A[A > 0].min() > 1e9
    # interleaved in index, and the fold order matters: the reversed fold gives other bits
    assert (np.diff(labels) != 0).sum() > 50
    rev = oc.cluster_areas(labels, A, len(counts), reverse=True)
    big = counts > 1
    assert (rev[big] != area[big]).all() and (rev[~big] == area[~big]).all()
    np.testing.assert_allclose(rev, area, rtol=1e-12)


@pytest.mark.parametrize("n", cs.MASK_SIZES)
@pytest.mark.parametrize("kind", cs.MASK_KINDS)
def test_remove_triangles_by_mask(n, kind):
    P, T, m = cs.mask_case(n, kind)
    P2, T2 = oc.remove_triangles_by_mask(P, T, m)
    assert P2 is not None and len(P2) == len(P)
    assert len(T2) == n - int((m != 0).sum())
    np.testing.assert_array_equal(T2, np.array([t for t, x in zip(T.tolist(), m) if not x], dtype=np.int32).reshape(-1, 3))


def test_remove_unreferenced_vertices():
    for name, (P, T) in cs.unreferenced_cases().items():
        P2, T2 = oc.remove_unreferenced_vertices(P, T)
        used = sorted(set(T.reshape(-1).tolist()))
        np.testing.assert_array_equal(P2, P[used], err_msg=name)
        np.testing.assert_array_equal(P2[T2].reshape(-1, 3), P[T].reshape(-1, 3), err_msg=name)
        if name.startswith("all_referenced") and len(T):
            assert len(P2) == len(P)
        if name.startswith("holes") and len(T):
            assert len(P2) < len(P)
    assert len(oc.remove_unreferenced_vertices(*cs.unreferenced_cases()["none_referenced"])[0]) == 0
    assert len(oc.remove_unreferenced_vertices(*cs.unreferenced_cases()["last_only"])[0]) == 1


def test_select_components_on_two_spheres():
    P, N = cs.two_spheres()
    r = mo.poisson(P, N, 5)
    V, T = mo.remove_vertices_by_mask(r["vertices"], r["triangles"], r["densities"] < mo.quantile(r["densities"], 0.02))
    labels, counts, _ = oc.cluster_connected_triangles(T, len(V))
    assert len(counts) == 2 and counts.max() > 5 * counts.min() > 0      # the two-sphere mesh has two components
    V1, T1 = oc.select_components(V, T, keep_largest=True)
    assert len(T1) == counts.max() and len(V1) < len(V)
    assert oc.cluster_connected_triangles(T1, len(V1))[1].tolist() == [counts.max()]
    V2, T2 = oc.select_components(V, T, min_triangles=int(counts.min()) + 1)
    np.testing.assert_array_equal(T1, T2)
    np.testing.assert_array_equal(V1, V2)
    V3, T3 = oc.select_components(V, T, min_triangles=int(counts.max()) + 1, keep_largest=True)
    assert len(V3) == 0 and len(T3) == 0


@pytest.mark.parametrize("name", sorted(SIMPLIFY))
def test_simplify_equals_the_plain_loop(name):
    P, T, vs = SIMPLIFY[name]
    V1, T1 = oc.simplify_vertex_clustering(P, T, vs)
    V2, T2 = oc.simplify_loop(P, T, vs)
    np.testing.assert_array_equal(V1, V2)
    np.testing.assert_array_equal(T1, T2)
    assert T1.dtype == np.int32 and V1.dtype == np.float64


def test_simplify_preconditions():
    c = SIMPLIFY
    P, T, vs = c["on_a_face"]
    g = (P[:, 0] - (P[:, 0].min() - vs * 0.5)) / vs
    assert g[1] == 1.0 and g[5] < 1.0                      # exactly on the face: the upper voxel
    V, T2 = oc.simplify_vertex_clustering(P, T, vs)
    assert oc.voxel_coords(P, vs)[[1, 5], 0].tolist() == [1, 0] and len(V) == 5
    P, T, vs = c["negative_coordinates"]
    assert (P < 0).any() and (P > 0).any()
    V, T2 = oc.simplify_vertex_clustering(*c["one_voxel"])
    assert len(V) == 1 and len(T2) == 0
    P, T, vs = c["own_voxels"]
    info = {}
    V, T2 = oc.simplify_vertex_clustering(P, T, vs, info)
    np.testing.assert_array_equal(V, P)                    # every vertex alone: numbering and positions unchanged
    assert min(info["rotations"]) > 0 and info["collapsed"] == 0
    # (1, 2, 3) three times (two dropped), its opposite kept, first occurrences in input order although
    # (1, 2, 3) sorts before (5, 6, 7)
    assert T2.tolist() == [[5, 6, 7], [1, 2, 3], [1, 3, 2], [4, 9, 8], [11, 20, 26], [11, 26, 20]]
    P, T, vs = c["vertex_0_highest_key"]
    vox = oc.voxel_coords(P, vs)
    assert (vox[0] == vox.max(0)).all()
    V, T2 = oc.simplify_vertex_clustering(P, T, vs)
    np.testing.assert_array_equal(V[0], P[0])              # first encounter, not key order, numbers the voxels
    P, T, vs = c["unreferenced_alone"]
    V, T2 = oc.simplify_vertex_clustering(P, T, vs)
    assert len(V) == 6 and T2.tolist() == [[0, 1, 2], [1, 2, 3]] and sorted(set(T2.reshape(-1).tolist())) == [0, 1, 2, 3]
    np.testing.assert_array_equal(V[0], (np.zeros(3) + P[0] + P[8]) / 2.0)   # an unreferenced member counts
    for n in (4095, 4096, 4097):
        P, T, vs = c[f"strip_{n}"]
        info = {}
        V, T2 = oc.simplify_vertex_clustering(P, T, vs, info)
        assert len(T) == n and info["collapsed"] > 0 and 0 < len(T2) < n
    # the strips above lose triangles before the triple sort (4073 .. 4088 rows reach it: one tile of 4096); these
    # bring exactly n rows to it, with equal third indices on both sides of row 4096 before and after its first sort
    for n in (4095, 4096, 4097):
        P, T, vs = c[f"live_{n}"]
        info = {}
        V, T2 = oc.simplify_vertex_clustering(P, T, vs, info)
        np.testing.assert_array_equal(V, P)
        assert len(T) == n and info["collapsed"] == 0 and info["duplicates"] > 500 and len(T2) == n - info["duplicates"]
        rot = np.array([np.roll(t, -int(np.argmin(t))) for t in T])
        assert rot[0].tolist() == rot[n - 1].tolist() == [5, 6, len(P) - 1] and (rot[1:n - 1, 2] < len(P) - 1).all()
        assert np.sort(rot[:, 2], kind="stable")[-2:].tolist() == [len(P) - 1] * 2


def test_simplify_errors():
    P, T, _ = SIMPLIFY["on_a_face"]
    for vs in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="voxel_size <= 0."):
            oc.simplify_vertex_clustering(P, T, vs)
    with pytest.raises(ValueError, match="voxel_size is too small."):
        oc.simplify_vertex_clustering(P, T, 1e-10)
    with pytest.raises(ValueError, match="2e6 voxels per axis"):
        oc.simplify_vertex_clustering(P, T, 1e-7)
    bad = P.copy()
    bad[2, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        oc.simplify_vertex_clustering(bad, T, 0.5)


@pytest.mark.parametrize("steps", [1.5, 2.0, 4.0])
def test_simplify_poisson_sphere(steps):
    V, T, h = cs.poisson_sphere()
    info = {}
    V2, T2 = oc.simplify_vertex_clustering(V, T, steps * h, info)
    assert 0 < len(T2) < len(T) and len(V2) < len(V)
    assert len(T) == len(T2) + info["collapsed"] + info["duplicates"]
    assert info["collapsed"] > 0 and min(info["rotations"]) > 0
    if steps < 4.0:     # the triple sort and the compaction after it run over more than one tile of 4096 rows
        assert len(T) - info["collapsed"] > 4096 and len(T2) > 4096
    if steps == 2.0:
        assert info["duplicates"] > 0 and not mo.edge_census(T2)[0]     # not closed: that is the algorithm
