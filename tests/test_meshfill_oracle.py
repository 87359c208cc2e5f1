"""tests/meshfill_oracle.py (the definition the GPU hole filling is checked against) against a second, naive
restatement: every loop walked side by side with Python loops, the same centroid rule in Python integers, the same
output order.  Without this the oracle would be pinned by itself alone.  CPU only."""
import math

import numpy as np
import pytest

from tests import meshcheck_oracle as ko
from tests import meshfill_cases as fc
from tests import meshfill_oracle as fo

CASES = fc.cases()
RUNS = fc.runs()


def naive_sides(T):
    """The directed sides whose undirected edge occurs once, by counting in a dict."""
    seen = {}
    for tri in T.tolist():
        for k in range(3):
            a, b = tri[k], tri[(k + 1) % 3]
            seen.setdefault((min(a, b), max(a, b)), []).append((a, b))
    return [s[0] for s in seen.values() if len(s) == 1]


def naive_components(sides):
    """-> [(label, sides of the component, simple)] in ascending label, by a search over the vertices."""
    out_of, into, touch = {}, {}, {}
    for a, b in sides:
        out_of.setdefault(a, []).append((a, b))
        into.setdefault(b, []).append((a, b))
        for v in (a, b):
            touch.setdefault(v, []).append((a, b))
    done, comps = set(), []
    for seed in sorted(touch):
        if seed in done:
            continue
        verts, stack = {seed}, [seed]
        while stack:
            for a, b in touch[stack.pop()]:
                for v in (a, b):
                    if v not in verts:
                        verts.add(v)
                        stack.append(v)
        done |= verts
        mine = [s for s in sides if s[0] in verts]
        simple = all(len(out_of.get(v, [])) == 1 and len(into.get(v, [])) == 1 for v in verts)
        comps.append((min(verts), mine, simple, verts, out_of))
    return comps


def naive_extent(P, verts):
    Q = P[sorted(verts)]
    d = Q.max(0) - Q.min(0)
    return math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def naive_fill(P, T, hole_size=None, max_hole_edges=None):
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    T = np.asarray(T, dtype=np.int32).reshape(-1, 3)
    V = len(P)
    comps = naive_components(naive_sides(T))
    counts = dict.fromkeys(fo.COUNT_KEYS, 0)
    counts["boundary_sides"] = sum(len(c[1]) for c in comps)
    if not comps:
        return P, T, counts
    lo = P.min(0)
    e = float((P.max(0) - lo).max())
    s = 1.0 if e == 0.0 else 2.0 ** (40 - max(math.frexp(e)[1], -983))
    new_v, new_t = [], []
    for label, sides, simple, verts, out_of in comps:
        counts["components"] += 1
        if not simple:
            counts["skipped_not_simple"] += 1
            continue
        counts["simple_loops"] += 1
        n = len(sides)
        if n < 3 or n > 2 ** 22 or (max_hole_edges is not None and n > max_hole_edges) or \
                (hole_size is not None and not naive_extent(P, verts) <= hole_size):
            counts["skipped_by_limit"] += 1
            continue
        counts["filled"] += 1
        walk = [label]                                    # the cycle, from the label along the sides
        while len(walk) < n:
            walk.append(out_of[walk[-1]][0][1])
        assert out_of[walk[-1]][0][1] == label and len(set(walk)) == n
        if n == 3:
            a, b, c = walk
            new_t.append((a, (a, c, b)))
            continue
        S = [0, 0, 0]
        for v in walk:
            for k in range(3):
                S[k] += int(np.rint((P[v, k] - lo[k]) * s))
        centre = V + len(new_v)                           # the components come in ascending label
        new_v.append([lo[k] + (float(S[k]) / float(n)) / s for k in range(3)])
        for i, a in enumerate(walk):
            new_t.append((a, (walk[(i + 1) % n], a, centre)))
    new_t.sort(key=lambda x: x[0])
    counts["new_vertices"], counts["new_triangles"] = len(new_v), len(new_t)
    Vo = np.concatenate([P, np.array(new_v, dtype=np.float64).reshape(-1, 3)])
    To = np.concatenate([T, np.array([t for _, t in new_t], dtype=np.int32).reshape(-1, 3)])
    return Vo, To, counts


def _same(got, want):
    for g, w in zip(got[:2], want[:2]):
        assert g.dtype == w.dtype and g.shape == w.shape
        np.testing.assert_array_equal(g, w)
    assert got[2] == want[2]


@pytest.mark.parametrize("run", RUNS, ids=fc.run_id)
def test_oracle_equals_the_naive_walk(run):
    name, size, edges = run
    P, T = CASES[name]
    size, edges = fc.limits(name, (size, edges))
    _same(fc.reference(run), naive_fill(P, T, size, edges))


@pytest.mark.parametrize("name", sorted(CASES))
def test_boundary_loops_equal_the_naive_components(name):
    P, T = CASES[name]
    got = fc.reference_loops(name)
    comps = naive_components(naive_sides(T))
    assert got["label"].dtype == np.int32 and got["size"].dtype == np.int64 and got["simple"].dtype == bool
    assert got["extent"].dtype == np.float64
    assert got["label"].tolist() == [c[0] for c in comps]
    assert got["size"].tolist() == [len(c[1]) for c in comps]
    assert got["simple"].tolist() == [c[2] for c in comps]
    assert got["extent"].tolist() == [naive_extent(P, c[3]) for c in comps]
    no_p = fo.boundary_loops(None, T, n_vertices=len(P))
    assert set(no_p) == {"label", "size", "simple"} and all((no_p[k] == got[k]).all() for k in no_p)


def test_what_the_cases_are_for():
    """The shapes are what their names say: the rules they are meant to reach are reached."""
    def counts(name, size=None, edges=None):
        return fc.reference((name, size, edges))[2]
    assert counts("single_triangle") == dict(components=1, simple_loops=1, filled=1, skipped_not_simple=0,
                                             skipped_by_limit=0, new_vertices=0, new_triangles=1, boundary_sides=3)
    V, T, _ = fc.reference(("single_triangle", None, None))
    assert T.tolist() == [[0, 1, 2], [0, 2, 1]]
    V, T, c = fc.reference(("tetrahedron_minus_face", None, None))
    assert len(V) == 4 and c["new_triangles"] == 1 and ko.check(V, T)["watertight"]
    assert {ko_rot(t) for t in T.tolist()} == {ko_rot(t) for t in fc.kc.tetrahedron()[1].tolist()}
    V, T, c = fc.reference(("cube_minus_face", None, None))
    assert c["new_vertices"] == 1 and c["new_triangles"] == 4 and V[8].tolist() == [1.0, 0.5, 0.5]
    chk = ko.check(V, T)
    assert chk["watertight"] and chk["volume"] == 1.0 and chk["signed_volume"] > 0.0
    # the cylinder: loops of 7 and 14 sides whose labels come in both orders
    assert sorted(fc.reference_loops("cylinder")["size"].tolist()) == [7, 14]
    orders = {tuple(fc.reference_loops(n)["size"].tolist()) for n in ("cylinder_shuffled_1", "cylinder_shuffled_2")}
    assert orders == {(7, 14), (14, 7)}
    assert counts("cylinder")["filled"] == 2 and ko.check(*fc.reference(("cylinder", None, None))[:2])["watertight"]
    assert counts("cylinder", None, 13) == dict(components=2, simple_loops=2, filled=1, skipped_not_simple=0,
                                                skipped_by_limit=1, new_vertices=1, new_triangles=7, boundary_sides=21)
    assert counts("cylinder", None, 6)["filled"] == 0
    for k in (0, 1):                                   # hole_size is inclusive; one ulp below skips that loop
        n = int(fc.reference_loops("cylinder")["size"][k])
        e = np.sort(fc.reference_loops("cylinder")["extent"])
        at, below = counts("cylinder", f"extent:{k}"), counts("cylinder", f"below:{k}")
        assert at["new_triangles"] - below["new_triangles"] == n and e[0] < e[1]
    # two holes that touch are one component that is not simple; the hole elsewhere and the rim are filled
    loops = fc.reference_loops("figure_eight")
    assert loops["simple"].tolist().count(False) == 1 and sorted(loops["size"].tolist()) == [4, 8, 22]
    assert counts("figure_eight")["filled"] == 2 and counts("figure_eight", None, 4)["filled"] == 1
    assert counts("two_cones_one_apex")["filled"] == 2
    assert counts("fans_65_at_hub") | dict(boundary_sides=0) == dict(
        components=1, simple_loops=0, filled=0, skipped_not_simple=1, skipped_by_limit=0, new_vertices=0,
        new_triangles=0, boundary_sides=0)
    c = counts("degenerate_in_run")                    # the self-loops 0 -> 0 and 4 -> 4 sit at vertices that are not simple
    assert c["filled"] == 0 and c["skipped_not_simple"] == c["components"] > 0
    c = counts("aab")                                  # a self-loop alone: a simple loop of one side, never eligible
    assert c["simple_loops"] == c["skipped_by_limit"] >= 1 and c["filled"] == 0
    assert 1 in fc.reference_loops("aab")["size"].tolist()
    c = counts("book_3")                               # the spine has three sides: no boundary; the pages' free edges
    assert c["boundary_sides"] == 6 and c["components"] == 1 and c["skipped_not_simple"] == 1
    # A Mobius strip's rim is one cycle of edges but NOT a simple loop as defined: whatever the windings, the
    # inconsistent edges cut the strip from rim to rim, and at the cut's two ends the sides' directions turn round
    # (two sides enter one vertex, two leave the other).  It is skipped, as any component with such a vertex.
    for name, n in (("mobius_5", 5), ("mobius_257", 257)):
        loops = fc.reference_loops(name)
        assert loops["size"].tolist() == [2 * n] and loops["simple"].tolist() == [False]
        assert counts(name)["skipped_not_simple"] == 1 and counts(name)["filled"] == 0
    assert counts("cone_5000")["new_triangles"] == 5000
    for name in ("empty", "vertices_only", "tetrahedron", "cube", "torus_64x65", "klein_8x9", "aaa"):
        V, T, c = fc.reference((name, None, None))
        assert not any(c.values())
        np.testing.assert_array_equal(V, CASES[name][0])
        np.testing.assert_array_equal(T, CASES[name][1])


def ko_rot(t):
    from tests import meshclean_oracle as mco
    return mco._rotate(tuple(t))


@pytest.mark.parametrize("run", RUNS, ids=fc.run_id)
def test_invariants(run):
    """What a fill leaves: the skipped components' sides as the only boundary, consistency and vertex manifoldness
    as before, the old mesh as a prefix, the skipped components as the result's boundary loops."""
    name, size, edges = run
    P, T = CASES[name]
    V, To, c = fc.reference(run)
    np.testing.assert_array_equal(V[: len(P)], P)
    np.testing.assert_array_equal(To[: len(T)], T)
    assert len(V) == len(P) + c["new_vertices"] and len(To) == len(T) + c["new_triangles"]
    before, after = ko.check(P, T), ko.check(V, To)
    loops = fc.reference_loops(name)
    assert before["boundary_edges"] == c["boundary_sides"] == int(loops["size"].sum())
    assert after["consistent"] == before["consistent"]
    assert after["vertex_manifold"] == before["vertex_manifold"]
    assert after["non_manifold_edges"] == before["non_manifold_edges"]
    left = fo.boundary_loops(V, To)
    assert after["boundary_edges"] == int(left["size"].sum()) == c["boundary_sides"] - c["new_triangles"] * 1 \
        - 2 * (c["filled"] - c["new_vertices"])
    if size is None and edges is None:
        skipped = ~loops["simple"] | (loops["size"] < 3)
        for k in left:
            np.testing.assert_array_equal(left[k], loops[k][skipped])
        if c["components"] == c["filled"] and before["edge_manifold"] and before["vertex_manifold"] \
                and before["consistent"]:
            assert after["watertight"]


def test_errors():
    P, T = CASES["cube_minus_face"]
    for size, edges in fc.BAD_LIMITS:
        with pytest.raises(ValueError):
            fo.fill_holes(P, T, hole_size=size, max_hole_edges=edges)
    bad = P.copy()
    bad[3, 2] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        fo.fill_holes(bad, T)
    with pytest.raises(IndexError, match="triangle index out of range"):
        fo.fill_holes(P[:7], T)
