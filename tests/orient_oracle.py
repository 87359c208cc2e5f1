"""CPU restatement of the consistent tangent-plane normal orientation
(csrc/slorient.inl states the rules; include/slgpu.h repeats them): Kruskal
over the slots in (weight, slot) order with union-find, then a walk of the
forest from every component's root.  The GPU finds the same forest with Boruvka
rounds; the order is strict and total, so the forest is unique as a set of
slots and the two are compared bit for bit.  Test infrastructure only.

Also the generators the orientation tests share: ``torus`` (a surface that is
not star-shaped about its centroid, so the radial orientation fails on it) and
``hybrid`` (the brute-force restatement of sl_radius_search for small clouds).
"""
from __future__ import annotations

import numpy as np


def torus(n, seed, R=1.0, r=0.4, centre=(0.0, 0.0, 0.0)):
    """-> (points, outward unit normals) f64 [n, 3]: area-uniform on the torus about the z axis."""
    rng = np.random.default_rng(seed)
    u = rng.random(n) * 2.0 * np.pi
    v = np.empty(0)
    while len(v) < n:  # the area element is proportional to R + r cos v
        c = rng.random(2 * n) * 2.0 * np.pi
        v = np.concatenate([v, c[rng.random(2 * n) * (R + r) < R + r * np.cos(c)]])
    v = v[:n]
    N = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], 1)
    ring = np.stack([R * np.cos(u), R * np.sin(u), np.zeros(n)], 1)
    return ring + r * N + np.asarray(centre, dtype=np.float64), N


def hybrid(points, radius, k):
    """sl_radius_search by brute force -> (idx int32 [n, k], cnt int32 [n]): per point the points with
    ((dx^2 + dy^2) + dz^2) < radius^2 (itself included), ascending (d2, index), the first k; unused entries -1."""
    P = np.ascontiguousarray(points, dtype=np.float64)
    n = len(P)
    idx = np.full((n, k), -1, np.int32)
    cnt = np.zeros(n, np.int32)
    r2 = float(radius) * float(radius)
    for i in range(n):
        d = P - P[i]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        near = np.nonzero(d2 < r2)[0]
        near = near[np.lexsort((near, d2[near]))][:k]
        idx[i, : len(near)] = near
        cnt[i] = len(near)
    return idx, cnt


def edges(normals, idx, cnt):
    """Every edge candidate -> (slot int64, u, v, w f64, flip bool), in slot order."""
    N = np.ascontiguousarray(normals, dtype=np.float64)
    idx = np.asarray(idx)
    n, k = idx.shape
    assert n * k < 2 ** 32
    j = np.arange(k)[None, :]
    rows = np.broadcast_to(np.arange(n, dtype=np.int64)[:, None], (n, k))
    ok = (j < np.asarray(cnt).reshape(n, 1)) & (idx != rows)
    u = rows[ok]
    v = idx[ok].astype(np.int64)
    slot = (rows * k + j)[ok]
    a, b = N[u], N[v]
    dot = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
    w = 1.0 - np.abs(dot)
    w = np.where(w > 0.0, w, 0.0)
    return slot, u, v, w, dot < 0.0


def _find_all(parent, x):
    r = parent[x]
    while True:
        rr = parent[r]
        if np.array_equal(rr, r):
            return r
        r = rr


def kruskal(n, slot, u, v, w):
    """The minimum spanning forest over (w, slot) -> positions (into the edge arrays) of its edges."""
    order = np.lexsort((slot, w))
    parent = np.arange(n, dtype=np.int64)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    tree = []
    pos, chunk = 0, 1024
    while pos < len(order) and len(tree) < n - 1:
        e = order[pos: pos + chunk]
        # edges inside a component at the chunk's start stay inside: drop them at once
        e = e[_find_all(parent, u[e]) != _find_all(parent, v[e])]
        for t in e.tolist():
            a, b = find(int(u[t])), find(int(v[t]))
            if a != b:
                parent[max(a, b)] = min(a, b)
                tree.append(t)
        parent = _find_all(parent, np.arange(n, dtype=np.int64))
        pos += chunk
        chunk = min(2 * chunk, 1 << 17)
    return np.array(tree, dtype=np.int64)


def orient(points, normals, idx, cnt):
    """-> (oriented normals f64 [n, 3], the forest's slots ascending int64, the number of components)."""
    P = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    N = np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, 3)
    n = len(P)
    if n == 0:
        return N.copy(), np.zeros(0, np.int64), 0
    slot, u, v, w, flip = edges(N, idx, cnt)
    tree = kruskal(n, slot, u, v, w)
    adj = [[] for _ in range(n)]
    for t in tree.tolist():
        a, b, f = int(u[t]), int(v[t]), bool(flip[t])
        adj[a].append((b, f))
        adj[b].append((a, f))
    # components, then per component its root: the largest z + 0.0, the lowest index on ties
    comp = np.full(n, -1, np.int64)
    members = []
    for s in range(n):
        if comp[s] >= 0:
            continue
        comp[s] = len(members)
        stack, mine = [s], [s]
        while stack:
            a = stack.pop()
            for b, _ in adj[a]:
                if comp[b] < 0:
                    comp[b] = comp[s]
                    stack.append(b)
                    mine.append(b)
        members.append(np.array(sorted(mine)))
    z = P[:, 2] + 0.0
    neg = np.zeros(n, bool)
    for mine in members:
        root = int(mine[np.argmax(z[mine])])  # argmax: the first of the largest
        seen = {root}
        neg[root] = N[root, 2] < 0.0
        stack = [root]
        while stack:
            a = stack.pop()
            for b, f in adj[a]:
                if b not in seen:
                    seen.add(b)
                    neg[b] = neg[a] ^ f
                    stack.append(b)
    out = N.copy()
    out[neg] = -out[neg]
    return out, np.sort(slot[tree]), len(members)


def radial(points, normals):
    """The centroid-radial orientation: a normal is negated where it points towards the centroid."""
    P = np.asarray(points, dtype=np.float64)
    N = np.asarray(normals, dtype=np.float64)
    inward = ((P - P.mean(0)) * N).sum(1) < 0.0
    return np.where(inward[:, None], -N, N)


def agreement(normals, outward):
    """The share of normals on the outward side."""
    return float(((np.asarray(normals) * np.asarray(outward)).sum(1) > 0.0).mean())
