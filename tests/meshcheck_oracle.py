"""CPU restatement of the mesh checks of csrc/slmeshcheck.inl, in NumPy: the definition.

Open3D's is_edge_manifold, is_vertex_manifold, is_orientable, is_watertight,
get_non_manifold_edges / _vertices, orient_triangles, get_surface_area,
get_volume, remove_degenerate_triangles and remove_duplicated_triangles in the
order-free forms the kernels compute.  Open3D is not installed here, so parity
with it is UNPINNED and its loops are quoted from memory: this file is what the
GPU is checked against, exactly.  The vertex test and the orientation have a
second, sequential form each (Open3D's loops: the search over a vertex's link
graph, the breadth-first walk that refuses a directed edge twice) that the CPU
tests show equal to the order-free one.

Sides: (a, b, c) has a->b, b->c, c->a; a side's key is min V + max and its
direction bit from < to.  A triangle with two equal indices is degenerate: it
still gives its three sides to the edge counts and takes no part in the vertex
test.
"""
from __future__ import annotations

import numpy as np

from tests import meshclean_oracle as mco
from tests.plane_oracle import ordered_sum

_tris = mco._tris
check_indices = mco.check_indices


def sides(triangles, n_vertices):
    """-> (keys int64 [T, 3], direction bits bool [T, 3]) of a->b, b->c, c->a."""
    T = _tris(triangles)
    a, b = T, np.roll(T, -1, 1)
    return np.minimum(a, b) * int(n_vertices) + np.maximum(a, b), a < b


def degenerate(triangles):
    T = _tris(triangles)
    return (T[:, 0] == T[:, 1]) | (T[:, 1] == T[:, 2]) | (T[:, 2] == T[:, 0])


def _sorted_sides(T, n_vertices):
    """The sides in stable key order -> (keys, triangle, direction bit, corner from, corner to) per entry."""
    keys, dirs = sides(T, n_vertices)
    val = np.arange(3 * len(T))
    order = np.argsort(keys.reshape(-1), kind="stable")
    val = val[order]
    k = val % 3
    return keys.reshape(-1)[order], val // 3, dirs.reshape(-1)[order], val, val - k + (k + 1) % 3


def _runs(keys):
    """-> (the first position of every run, its length)."""
    if len(keys) == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    head = np.ones(len(keys), dtype=bool)
    head[1:] = keys[1:] != keys[:-1]
    start = np.nonzero(head)[0]
    return start, np.diff(np.append(start, len(keys)))


def edge_counts(triangles, n_vertices) -> dict:
    """The distinct edges, those of one side, of three or more sides, and of two sides with equal direction bits."""
    T = check_indices(triangles, n_vertices)
    keys, _, dirs, _, _ = _sorted_sides(T, n_vertices)
    start, m = _runs(keys)
    two = start[m == 2]
    return {"edges": len(start), "boundary_edges": int((m == 1).sum()), "non_manifold_edges": int((m >= 3).sum()),
            "inconsistent_edges": int((dirs[two] == dirs[two + 1]).sum())}


def get_non_manifold_edges(triangles, n_vertices, allow_boundary_edges=True):
    """-> int32 [E, 2] rows (min, max) in ascending key order."""
    T = check_indices(triangles, n_vertices)
    keys, _, _, _, _ = _sorted_sides(T, n_vertices)
    start, m = _runs(keys)
    pick = (m >= 3) if allow_boundary_edges else (m != 2)
    k = keys[start[pick]]
    V = max(int(n_vertices), 1)
    return np.stack([k // V, k % V], 1).astype(np.int32).reshape(-1, 2)


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def get_non_manifold_vertices(triangles, n_vertices):
    """The corner form -> int32 [M], ascending.  A corner is (t, k), index 3 t + k; two corners at one vertex are
    joined iff their (non-degenerate) triangles share an edge that contains it; a vertex whose corners fall into
    more than one class is non-manifold."""
    T = check_indices(triangles, n_vertices)
    live = ~degenerate(T)
    keys, tri, _, cf, ct = _sorted_sides(T, n_vertices)
    sel = live[tri]
    keys, cf, ct = keys[sel], cf[sel], ct[sel]      # the runs among the non-degenerate triangles
    flat = T.reshape(-1)
    parent = list(range(3 * len(T)))
    for i in np.nonzero(keys[1:] == keys[:-1])[0] + 1:
        for v in (flat[cf[i]], flat[ct[i]]):          # the two ends; each entry has one corner at either
            a = cf[i] if flat[cf[i]] == v else ct[i]
            b = cf[i - 1] if flat[cf[i - 1]] == v else ct[i - 1]
            a, b = _find(parent, int(a)), _find(parent, int(b))
            if a != b:
                parent[max(a, b)] = min(a, b)
    classes = np.zeros(int(n_vertices), dtype=np.int64)
    for x in np.nonzero(np.repeat(live, 3))[0]:
        if parent[x] == x:
            classes[flat[x]] += 1
    return np.nonzero(classes > 1)[0].astype(np.int32)


def get_non_manifold_vertices_link(triangles, n_vertices):
    """Open3D's GetNonManifoldVertices: per vertex the graph of the edges opposite to it in its triangles (its
    link); non-manifold iff a search from one link vertex does not reach them all.  For meshes without degenerate
    triangles only."""
    T = check_indices(triangles, n_vertices)
    if degenerate(T).any():
        raise ValueError("the link form is defined without degenerate triangles only")
    at = {}
    for t, tri in enumerate(T):
        for v in tri:
            at.setdefault(int(v), []).append(t)
    out = []
    for v in sorted(at):                 # a vertex of no triangle is skipped, as in Open3D
        link = {}
        for t in at[v]:
            a, b = (int(x) for x in T[t] if x != v)
            link.setdefault(a, set()).add(b)
            link.setdefault(b, set()).add(a)
        first = next(iter(link))
        seen, queue = {first}, [first]
        while queue:
            for w in link[queue.pop(0)]:
                if w not in seen:
                    seen.add(w)
                    queue.append(w)
        if len(seen) != len(link):
            out.append(v)
    return np.array(out, dtype=np.int32)


def _flip(T, flips):
    out = T.copy()
    out[flips] = T[flips][:, [0, 2, 1]]
    return out


def orient_triangles(triangles, n_vertices):
    """The order-free form -> (triangles int32 [T, 3], orientable).  Orientable iff no edge has three or more sides
    and the constraints flip(t1) ^ flip(t2) = (the two direction bits are equal), one per two-sided edge (of one
    triangle: the bits must differ; a two-sided loop {a, a} has the same direction twice whatever is flipped and is
    never satisfied), have a solution.  Components are connected through two-sided edges; the
    smallest triangle index of each keeps its winding; a flipped (a, b, c) is (a, c, b).  Not orientable: the
    triangles unchanged."""
    T = check_indices(triangles, n_vertices)
    keys, tri, dirs, _, _ = _sorted_sides(T, n_vertices)
    start, m = _runs(keys)
    ok = not (m >= 3).any()
    two = start[m == 2]
    t1, t2, rel = tri[two], tri[two + 1], dirs[two] == dirs[two + 1]
    own = t1 == t2
    loop = keys[two] % max(int(n_vertices), 1) == keys[two] // max(int(n_vertices), 1)   # {a, a}: no flip turns it
    if (rel & own).any() or loop.any():
        ok = False
    own = own | loop
    nb = [[] for _ in range(len(T))]
    for a, b, r in zip(t1[~own].tolist(), t2[~own].tolist(), rel[~own].tolist()):
        nb[a].append((b, r))
        nb[b].append((a, r))
    flip = np.full(len(T), -1, dtype=np.int64)
    for seed in range(len(T)):          # ascending: a component's smallest index is its seed
        if flip[seed] >= 0:
            continue
        flip[seed] = 0
        stack = [seed]
        while stack:
            t = stack.pop()
            for u, r in nb[t]:
                want = flip[t] ^ int(r)
                if flip[u] < 0:
                    flip[u] = want
                    stack.append(u)
                elif flip[u] != want:
                    ok = False
    if not ok:
        return T.astype(np.int32), False
    return _flip(T, flip == 1).astype(np.int32), True


def orient_triangles_sequential(triangles, n_vertices):
    """Open3D's OrientTriangles, seeded from the smallest unvisited index: breadth-first over shared edges; a
    triangle one of whose directed edges is taken already is flipped; no directed edge may then occur twice.
    -> (triangles, orientable); not orientable: the triangles unchanged."""
    T = check_indices(triangles, n_vertices)
    keys, _ = sides(T, n_vertices)
    by_edge = {}
    for t in range(len(T)):
        for k in keys[t]:
            by_edge.setdefault(int(k), []).append(t)
    out = T.copy()
    taken, visited = set(), np.zeros(len(T), dtype=bool)
    for seed in range(len(T)):
        if visited[seed]:
            continue
        queue = [seed]
        while queue:
            t = queue.pop(0)
            if visited[t]:
                continue
            visited[t] = True
            a, b, c = (int(x) for x in out[t])
            if (a, b) in taken or (b, c) in taken or (c, a) in taken:
                b, c = c, b
                out[t] = (a, b, c)
            for e in ((a, b), (b, c), (c, a)):
                if e in taken:
                    return T.astype(np.int32), False
                taken.add(e)
            for k in keys[t]:
                queue.extend(by_edge[int(k)])
    return out.astype(np.int32), True


def measures(vertices, triangles):
    """-> (A_t, W_t) f64 [T]: 0.5 sqrt((n0 n0 + n1 n1) + n2 n2) with n = (v1 - v0) x (v2 - v0), and ((x0 c0 + y0 c1)
    + z0 c2) / 6.0 with c = v1 x v2."""
    P = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    T = check_indices(triangles, len(P))
    if not np.isfinite(P).all():
        raise ValueError("non-finite vertex coordinates")
    p0, p1, p2 = P[T[:, 0]], P[T[:, 1]], P[T[:, 2]]
    c0 = p1[:, 1] * p2[:, 2] - p1[:, 2] * p2[:, 1]
    c1 = p1[:, 2] * p2[:, 0] - p1[:, 0] * p2[:, 2]
    c2 = p1[:, 0] * p2[:, 1] - p1[:, 1] * p2[:, 0]
    return mco.triangle_areas(P, T), ((p0[:, 0] * c0 + p0[:, 1] * c1) + p0[:, 2] * c2) / 6.0


def check(vertices, triangles, n_vertices=None) -> dict:
    """mesh.check's dict."""
    P = None if vertices is None else np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    V = len(P) if n_vertices is None else int(n_vertices)
    T = check_indices(triangles, V)
    c = {"vertices": V, "triangles": len(T)}
    c.update(edge_counts(T, V))
    c["non_manifold_vertices"] = len(get_non_manifold_vertices(T, V))
    c["degenerate_triangles"] = int(degenerate(T).sum())
    c["edge_manifold"] = c["non_manifold_edges"] == 0
    c["edge_manifold_closed"] = c["edge_manifold"] and c["boundary_edges"] == 0
    c["vertex_manifold"] = c["non_manifold_vertices"] == 0
    c["orientable"] = orient_triangles(T, V)[1]
    c["consistent"] = c["inconsistent_edges"] == 0
    c["watertight"] = c["edge_manifold_closed"] and c["vertex_manifold"] and c["consistent"]
    c["area"] = c["volume"] = c["signed_volume"] = None
    if P is not None:
        A, W = measures(P, T)
        c["area"] = ordered_sum(A)
        if c["watertight"]:
            w = ordered_sum(W)
            c["volume"], c["signed_volume"] = abs(w), w
    return c


def get_surface_area(vertices, triangles) -> float:
    return ordered_sum(measures(vertices, triangles)[0])


def get_volume(vertices, triangles, signed=False) -> float:
    if not check(vertices, triangles)["watertight"]:
        raise ValueError("The mesh is not watertight, and the volume cannot be computed.")
    w = ordered_sum(measures(vertices, triangles)[1])
    return w if signed else abs(w)


def remove_degenerate_triangles(triangles, n_vertices):
    T = check_indices(triangles, n_vertices)
    return T[~degenerate(T)].astype(np.int32).reshape(-1, 3)


def remove_duplicated_triangles(triangles, n_vertices):
    """The first occurrence, in input order and as given, of every triple rotated by meshclean_oracle._rotate (the
    strictly smallest index first; the opposite winding is another triple)."""
    T = check_indices(triangles, n_vertices)
    seen, keep = set(), []
    for t in T:
        r = mco._rotate(tuple(int(x) for x in t))
        keep.append(r not in seen)
        seen.add(r)
    return T[np.array(keep, dtype=bool)].astype(np.int32).reshape(-1, 3)
