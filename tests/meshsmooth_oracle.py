"""CPU restatement of csrc/slmeshsmooth.inl, which states the rules: Open3D's
compute_adjacency_list, filter_smooth_simple, filter_smooth_laplacian and
filter_smooth_taubin for the vertices of a triangle mesh.  NumPy, exact: the GPU
results equal these bit for bit (tests/test_gpu_meshsmooth.py).

Two forms.  The first is the order-free one the device mirrors: the adjacency as
CSR from the sorted directed pairs, the filters vectorised over the vertices and
sequential over the neighbour rank, so every row is folded in ascending neighbour
index.  The second (``*_sets``) is Open3D's loops taken literally -- a Python set
per vertex, filled triangle by triangle -- with the one stated change that a set
is walked sorted (Open3D: the hash order of an unordered_set) and that a vertex
with an empty set keeps its position in the Laplacian step (Open3D: 0 / 0).
tests/test_meshsmooth_oracle.py holds the two equal on every case.

Open3D is not installed: parity with it is unpinned."""
from __future__ import annotations

import math

import numpy as np


def _check(T, nv):
    T = np.asarray(T, dtype=np.int64).reshape(-1, 3)
    if T.size and (T.min() < 0 or T.max() >= nv):
        raise IndexError("triangle index out of range")
    return T


def _vertices(P):
    P = np.ascontiguousarray(np.asarray(P, dtype=np.float64)).reshape(-1, 3)
    if not np.isfinite(P).all():
        raise ValueError("non-finite vertex coordinates")
    return P


def _arguments(iterations, *factors):
    if int(iterations) != iterations or iterations < 0:
        raise ValueError("iterations must be a non-negative integer")
    if not all(math.isfinite(f) for f in factors):
        raise ValueError("lambda_filter and mu must be finite")
    return int(iterations)


# ---- the order-free form ---------------------------------------------------------------------------------------
def adjacency_list(triangles, n_vertices, boundary=False):
    """-> (row_start int64 [V + 1], neighbours int32 [M][, boundary bool [V]])."""
    nv = int(n_vertices)
    T = _check(triangles, nv)
    a, b, c = T[:, 0], T[:, 1], T[:, 2]
    v = np.concatenate([a, a, b, b, c, c])
    w = np.concatenate([b, c, a, c, a, b])
    keys, runs = np.unique(v * nv + w, return_counts=True)   # below 2^62
    uv, uw = (keys // nv, keys % nv) if nv else (keys, keys)
    row_start = np.zeros(nv + 1, dtype=np.int64)
    row_start[1:] = np.cumsum(np.bincount(uv, minlength=nv))
    out = (row_start, uw.astype(np.int32))
    if boundary:
        bnd = np.zeros(nv, dtype=bool)
        bnd[uv[(runs == 1) & (uw != uv)]] = True
        out += (bnd,)
    return out


class _Rows:
    """The rows by rank: ranks[r] = (the vertices with more than r neighbours, their r-th neighbour)."""

    def __init__(self, T, nv, fixed_boundary, descending=False):
        row_start, nb, bnd = adjacency_list(T, nv, boundary=True)
        self.deg = np.diff(row_start)
        self.moving = ~bnd if fixed_boundary else np.ones(nv, dtype=bool)
        self.ranks = []
        for r in range(int(self.deg.max()) if nv else 0):
            idx = np.nonzero(self.deg > r)[0]
            at = row_start[idx + 1] - 1 - r if descending else row_start[idx] + r
            self.ranks.append((idx, nb[at].astype(np.int64)))


def _simple_step(P, rows):
    s = P.copy()
    for idx, j in rows.ranks:
        s[idx] = s[idx] + P[j]
    out = s / (1 + rows.deg).astype(np.float64)[:, None]
    return np.where(rows.moving[:, None], out, P)


def _laplacian_step(P, rows, factor):
    s = np.zeros_like(P)
    tw = np.zeros(len(P))
    for idx, j in rows.ranks:
        q = P[j]
        d = P[idx] - q
        dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        w = 1.0 / (dist + 1e-12)
        tw[idx] = tw[idx] + w
        s[idx] = s[idx] + w[:, None] * q
    move = rows.moving & (rows.deg > 0)
    out = P.copy()
    out[move] = P[move] + factor * (s[move] / tw[move][:, None] - P[move])
    return out


def filter_smooth_simple(vertices, triangles, iterations=1, fixed_boundary=False):
    P = _vertices(vertices)
    n = _arguments(iterations)
    rows = _Rows(_check(triangles, len(P)), len(P), fixed_boundary)
    P = P.copy()
    for _ in range(n):
        P = _simple_step(P, rows)
    return P


def filter_smooth_laplacian(vertices, triangles, iterations=1, lambda_filter=0.5, fixed_boundary=False,
                            descending=False):
    """``descending``: the rows folded from their last entry to their first -- NOT the definition; the tests use it
    to show that the order is part of the result."""
    P = _vertices(vertices)
    n = _arguments(iterations, lambda_filter)
    rows = _Rows(_check(triangles, len(P)), len(P), fixed_boundary, descending)
    P = P.copy()
    for _ in range(n):
        P = _laplacian_step(P, rows, float(lambda_filter))
    return P


def filter_smooth_taubin(vertices, triangles, iterations=1, lambda_filter=0.5, mu=-0.53, fixed_boundary=False):
    P = _vertices(vertices)
    n = _arguments(iterations, lambda_filter, mu)
    rows = _Rows(_check(triangles, len(P)), len(P), fixed_boundary)
    P = P.copy()
    for _ in range(n):
        P = _laplacian_step(P, rows, float(lambda_filter))
        P = _laplacian_step(P, rows, float(mu))
    return P


# ---- Open3D's loops, literally ----------------------------------------------------------------------------------
def _sets(T, nv):
    """ComputeAdjacencyList -> {vertex: set} for the vertices of a triangle, and the directed pairs' counts."""
    adj, count = {}, {}
    for a, b, c in _check(T, nv).tolist():
        for v, w in ((a, b), (a, c), (b, a), (b, c), (c, a), (c, b)):
            adj.setdefault(v, set()).add(w)
            count[(v, w)] = count.get((v, w), 0) + 1
    return adj, count


def _boundary_set(count):
    return {v for (v, w), n in count.items() if n == 1 and w != v}


def adjacency_list_sets(triangles, n_vertices, boundary=False):
    nv = int(n_vertices)
    adj, count = _sets(triangles, nv)
    row_start = np.zeros(nv + 1, dtype=np.int64)
    nb = []
    last = 0
    for v in sorted(adj):
        row_start[last + 1:v + 1] = len(nb)
        nb += sorted(adj[v])
        last = v
    row_start[last + 1:] = len(nb)
    out = (row_start, np.array(nb, dtype=np.int32))
    if boundary:
        bnd = np.zeros(nv, dtype=bool)
        bnd[sorted(_boundary_set(count))] = True
        out += (bnd,)
    return out


def _simple_step_sets(P, adj, fixed):
    out = [list(p) for p in P]
    for v, p in enumerate(P):
        if v in fixed:
            continue
        row = sorted(adj.get(v, ()))
        for a in range(3):
            s = p[a]
            for j in row:
                s = s + P[j][a]
            out[v][a] = s / float(1 + len(row))
    return out


def _laplacian_step_sets(P, adj, fixed, factor):
    out = [list(p) for p in P]
    for v, p in enumerate(P):
        row = sorted(adj.get(v, ()))
        if v in fixed or not row:
            continue
        s, tw = [0.0, 0.0, 0.0], 0.0
        for j in row:
            q = P[j]
            dx, dy, dz = p[0] - q[0], p[1] - q[1], p[2] - q[2]
            dist = math.sqrt((dx * dx + dy * dy) + dz * dz)
            w = 1.0 / (dist + 1e-12)
            tw = tw + w
            for a in range(3):
                s[a] = s[a] + w * q[a]
        for a in range(3):
            out[v][a] = p[a] + factor * (s[a] / tw - p[a])
    return out


def _filter_sets(vertices, triangles, steps, fixed_boundary):
    P = _vertices(vertices)
    adj, count = _sets(triangles, len(P))
    fixed = _boundary_set(count) if fixed_boundary else set()
    Q = P.tolist()
    for step in steps:
        Q = step(Q, adj, fixed)
    return np.array(Q, dtype=np.float64).reshape(-1, 3)


def filter_smooth_simple_sets(vertices, triangles, iterations=1, fixed_boundary=False):
    n = _arguments(iterations)
    return _filter_sets(vertices, triangles, [_simple_step_sets] * n, fixed_boundary)


def filter_smooth_laplacian_sets(vertices, triangles, iterations=1, lambda_filter=0.5, fixed_boundary=False):
    n = _arguments(iterations, lambda_filter)
    lam = float(lambda_filter)
    return _filter_sets(vertices, triangles, [lambda P, adj, fx: _laplacian_step_sets(P, adj, fx, lam)] * n,
                        fixed_boundary)


def filter_smooth_taubin_sets(vertices, triangles, iterations=1, lambda_filter=0.5, mu=-0.53, fixed_boundary=False):
    n = _arguments(iterations, lambda_filter, mu)
    lam, mu = float(lambda_filter), float(mu)
    pair = [lambda P, adj, fx: _laplacian_step_sets(P, adj, fx, lam),
            lambda P, adj, fx: _laplacian_step_sets(P, adj, fx, mu)]
    return _filter_sets(vertices, triangles, pair * n, fixed_boundary)


FILTERS = {"simple": filter_smooth_simple, "laplacian": filter_smooth_laplacian, "taubin": filter_smooth_taubin}
FILTERS_SETS = {"simple": filter_smooth_simple_sets, "laplacian": filter_smooth_laplacian_sets,
                "taubin": filter_smooth_taubin_sets}
