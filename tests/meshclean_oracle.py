"""CPU restatement of the mesh clean-up of csrc/slmeshclean.inl, in NumPy.

Open3D's cluster_connected_triangles, remove_triangles_by_mask,
remove_unreferenced_vertices and simplify_vertex_clustering(Average) in the
order-free forms the kernels compute.  Open3D is not installed here, so parity
with it is UNPINNED: this file is the reference the GPU is checked against, bit
for bit.  Each function has a second, sequential form (Open3D's loops: the
breadth-first labelling, the per-triangle simplification) that the CPU tests
show equal to the order-free one.
"""
from __future__ import annotations

import numpy as np

BLOCK = 64               # members per area block
INT_MAX = 2 ** 31 - 1


def _tris(triangles):
    return np.asarray(triangles, dtype=np.int64).reshape(-1, 3)


def check_indices(triangles, n_vertices):
    T = _tris(triangles)
    if len(T) and (T.min() < 0 or T.max() >= n_vertices):
        raise IndexError("triangle index out of range")
    return T


def edge_keys(triangles, n_vertices):
    """int64 [T, 3]: min V + max of {a, b}, {b, c}, {c, a}."""
    T = _tris(triangles)
    a, b = T, np.roll(T, -1, 1)
    return np.minimum(a, b) * int(n_vertices) + np.maximum(a, b)


def _roots(triangles, n_vertices):
    """The smallest triangle index of every triangle's component: union-find over the run neighbours of
    the sorted edge keys, the larger root hooked under the smaller."""
    T = _tris(triangles)
    keys = edge_keys(T, n_vertices).reshape(-1)
    vals = np.repeat(np.arange(len(T)), 3)
    order = np.argsort(keys, kind="stable")
    keys, vals = keys[order], vals[order]
    parent = list(range(len(T)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i in np.nonzero(keys[1:] == keys[:-1])[0] + 1:
        a, b = find(int(vals[i])), find(int(vals[i - 1]))
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(t) for t in range(len(T))], dtype=np.int64)


def triangle_areas(vertices, triangles):
    P = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    T = _tris(triangles)
    e1, e2 = P[T[:, 1]] - P[T[:, 0]], P[T[:, 2]] - P[T[:, 0]]
    n0 = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    n1 = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    n2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return 0.5 * np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)


def fold(values, reverse=False) -> float:
    """The members (in ascending triangle index) in blocks of 64 from the first; a block is a left fold from
    0.0 and so are the block sums.  ``reverse`` folds everything from the other end (a precondition check)."""
    v = [float(x) for x in values]
    if reverse:
        v = v[::-1]
    total = 0.0
    for at in range(0, len(v), BLOCK):
        s = 0.0
        for x in v[at:at + BLOCK]:
            s = s + x
        total = total + s
    return total


def cluster_areas(labels, areas, n_clusters, reverse=False):
    return np.array([fold(areas[labels == c], reverse) for c in range(n_clusters)], dtype=np.float64)


def cluster_connected_triangles(triangles, n_vertices, vertices=None):
    """-> (triangle_clusters int32 [T], cluster_n_triangles int64 [C], cluster_area f64 [C] | None)."""
    T = check_indices(triangles, n_vertices)
    if vertices is not None and not np.isfinite(np.asarray(vertices, dtype=np.float64)).all():
        raise ValueError("non-finite vertex coordinates")
    root = _roots(T, n_vertices)
    heads = root == np.arange(len(T))
    rank = np.cumsum(heads) - heads
    labels = rank[root].astype(np.int32)
    C = int(heads.sum())
    counts = np.bincount(labels, minlength=C).astype(np.int64)
    area = None if vertices is None else cluster_areas(labels, triangle_areas(vertices, T), C)
    return labels, counts, area


def cluster_sequential(triangles, n_vertices):
    """Open3D's loop: triangle indices ascending, breadth-first from the first unlabelled one."""
    T = check_indices(triangles, n_vertices)
    by_edge = {}
    keys = edge_keys(T, n_vertices)
    for t in range(len(T)):
        for k in keys[t]:
            by_edge.setdefault(int(k), []).append(t)
    labels = np.full(len(T), -1, dtype=np.int32)
    counts = []
    for t0 in range(len(T)):
        if labels[t0] >= 0:
            continue
        c = len(counts)
        labels[t0] = c
        queue, n = [t0], 0
        while queue:
            t = queue.pop(0)
            n += 1
            for k in keys[t]:
                for u in by_edge[int(k)]:
                    if labels[u] < 0:
                        labels[u] = c
                        queue.append(u)
        counts.append(n)
    return labels, np.array(counts, dtype=np.int64)


def remove_triangles_by_mask(vertices, triangles, mask):
    T = _tris(triangles)
    mask = np.asarray(mask).reshape(-1) != 0
    if len(mask) != len(T):
        raise ValueError("a mask entry per triangle is needed")
    return np.asarray(vertices, dtype=np.float64).reshape(-1, 3), T[~mask].astype(np.int32)


def remove_unreferenced_vertices(vertices, triangles):
    P = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    T = check_indices(triangles, len(P))
    ref = np.zeros(len(P), dtype=bool)
    ref[T.reshape(-1)] = True
    new = np.cumsum(ref) - ref
    return P[ref], new[T].astype(np.int32).reshape(-1, 3)


def select_components(vertices, triangles, keep_largest=False, min_triangles=None):
    P = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    labels, counts, _ = cluster_connected_triangles(triangles, len(P))
    keep = np.ones(len(counts), dtype=bool)
    if min_triangles is not None:
        keep &= counts >= int(min_triangles)
    if keep_largest and keep.any():
        c = np.where(keep, counts, -1)
        keep = np.zeros_like(keep)
        keep[int(np.argmax(c))] = True   # the first maximum: the lowest label on a tie
    _, T = remove_triangles_by_mask(P, triangles, ~keep[labels])
    return remove_unreferenced_vertices(P, T)


def voxel_coords(vertices, voxel_size):
    """-> int64 [V, 3]: floor((v - (min - vs/2)) / vs), with sl_voxel_downsample's limits and messages."""
    P = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    vs = float(voxel_size)
    if not vs > 0.0:
        raise ValueError("voxel_size <= 0.")
    if not np.isfinite(P).all():
        raise ValueError("non-finite vertex coordinates")
    lo = P.min(0) - vs * 0.5
    hi = P.max(0) + vs * 0.5
    if vs * INT_MAX < float((hi - lo).max()):
        raise ValueError("voxel_size is too small.")
    if (np.floor((P.max(0) - lo) / vs) > 2.0e6).any():
        raise ValueError("voxel grid exceeds 2e6 voxels per axis / 2^63 voxels")
    return np.floor((P - lo) / vs).astype(np.int64)


def _rotate(t):
    a, b, c = t
    if b < a and b < c:
        return b, c, a
    if c < a and c < b:
        return c, a, b
    return a, b, c


def simplify_loop(vertices, triangles, voxel_size):
    """The plain form: one vertex, then one triangle at a time, with dicts (Open3D's loops, except that a
    voxel's members are summed in ascending index and the triangles kept in first-occurrence order)."""
    P = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    T = check_indices(triangles, len(P))
    if len(P) == 0:
        return np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int32)
    vox = voxel_coords(P, voxel_size)
    index, sums, cnt, vmap = {}, [], [], []
    for v in range(len(P)):
        key = tuple(int(x) for x in vox[v])
        if key not in index:
            index[key] = len(sums)
            sums.append([0.0, 0.0, 0.0])
            cnt.append(0)
        i = index[key]
        for a in range(3):
            sums[i][a] = sums[i][a] + float(P[v, a])
        cnt[i] += 1
        vmap.append(i)
    out_v = np.array([[s[a] / float(n) for a in range(3)] for s, n in zip(sums, cnt)], dtype=np.float64)
    seen, out_t = set(), []
    for t in T:
        m = tuple(vmap[int(x)] for x in t)
        if m[0] == m[1] or m[1] == m[2] or m[2] == m[0]:
            continue
        m = _rotate(m)
        if m in seen:
            continue
        seen.add(m)
        out_t.append(m)
    return out_v.reshape(-1, 3), np.array(out_t, dtype=np.int32).reshape(-1, 3)


def simplify_vertex_clustering(vertices, triangles, voxel_size, info=None):
    """The vectorised form, as the kernels do it -> (vertices f64 [V', 3], triangles int32 [T', 3]).
    ``info`` (a dict) receives "collapsed", "duplicates" and "rotations" (how often each of the three occurred)."""
    P = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    T = check_indices(triangles, len(P))
    if len(P) == 0:
        return np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int32)
    vox = voxel_coords(P, voxel_size)
    _, inv = np.unique(vox, axis=0, return_inverse=True)     # voxels in key order
    inv = inv.reshape(-1)
    m = int(inv.max()) + 1
    first = np.full(m, len(P), dtype=np.int64)
    np.minimum.at(first, inv, np.arange(len(P)))             # the smallest member of every voxel
    head = np.zeros(len(P), dtype=bool)
    head[first] = True
    rank = np.cumsum(head) - head
    vmap = rank[first][inv]                                   # first-encounter numbering
    sums = np.zeros((m, 3))
    np.add.at(sums, vmap, P)                                  # unbuffered: ascending vertex index from 0.0
    out_v = sums / np.bincount(vmap, minlength=m).astype(np.float64)[:, None]
    M = vmap[T]
    ok = (M[:, 0] != M[:, 1]) & (M[:, 1] != M[:, 2]) & (M[:, 2] != M[:, 0])
    M = M[ok]
    shift = np.argmin(M, 1) if len(M) else np.zeros(0, dtype=np.int64)
    R = np.stack([M[np.arange(len(M)), (shift + s) % 3] for s in range(3)], 1) if len(M) else M
    # two stable sorts: by c, then by a V' + b; the head of every run is the first occurrence
    order = np.argsort(R[:, 2], kind="stable")
    order = order[np.argsort(R[order, 0] * m + R[order, 1], kind="stable")]
    S = R[order]
    is_head = np.ones(len(S), dtype=bool)
    is_head[1:] = (S[1:] != S[:-1]).any(1)
    keep = np.zeros(len(R), dtype=bool)
    keep[order[is_head]] = True
    if info is not None:
        info["collapsed"] = int((~ok).sum())
        info["duplicates"] = int(len(R) - keep.sum())
        info["rotations"] = np.bincount(shift, minlength=3).tolist()
    return out_v, R[keep].astype(np.int32).reshape(-1, 3)
