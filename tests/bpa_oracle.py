"""CPU restatement of csrc/slbpa.inl: ball-pivoting surface meshing in its
order-free form (Open3D's create_from_point_cloud_ball_pivoting is a sequential
front; Open3D is not installed: parity with it is unpinned, and this file is
the statement the kernel is checked against, exactly).

All arithmetic is f64, uncontracted, in the operation order written (NumPy's
elementwise products and sums are not fused).  d2(u, v) = ((dx dx + dy dy) +
dz dz), r2 = r r, R4 = 4 r2.

Candidate triangle at radius r: cloud indices i < j < k, p0, p1, p2 = P[i],
P[j], P[k], with
  neighbours     d2(p1, p0) < R4, d2(p2, p0) < R4, d2(p1, p2) < R4 (strict);
  circumcentre   a = d2(p1, p2), b = d2(p2, p0), c = d2(p0, p1),
                 wa = a ((b + c) - a), wb = b ((a + c) - b), wc = c ((a + b) - c),
                 s = (wa + wb) + wc > 0,
                 cc = (p0 (wa / s) + p1 (wb / s)) + p2 (wc / s),
                 h = r2 - d2(cc, p0) >= 0;
  normals        e1 = p1 - p0, e2 = p2 - p0, n = (e1y e2z - e1z e2y, e1z e2x -
                 e1x e2z, e1x e2y - e1y e2x), ln = sqrt((nx nx + ny ny) + nz nz)
                 > 0; dv = (nx Nv.x + ny Nv.y) + nz Nv.z for v = i, j, k: all
                 > 0 -> sign +1, all < 0 -> sign -1, else no candidate;
  ball centre    o = cc + (n / ln) (sign sqrt(h));
  emptiness      no point q other than i, j, k (by index) among the points with
                 d2(q, p0) < R4 has d2(q, o) < r2;
  winding        (i, j, k) for sign +1, (i, k, j) for sign -1;
  rank           the lexicographic order of the sorted triple (i, j, k).

Vertex classes against the mesh so far: 0 orphan (in no triangle), 1 border (on
an edge with exactly one triangle), 2 inner (used, on no such edge).

A pass at radius r over the mesh M (judged against that snapshot of M):
  1. the candidates whose three vertices are all non-inner;
  2. without those whose sorted triple is in M;
  3. without those that have an edge with two or more triangles in M;
  4. without those that have no edge in M, unless all three vertices are orphans;
  5. per edge, the survivors on it in rank order: only the first 2 -
     count_M(edge) stay; a triangle dropped at any of its edges is dropped (one
     application);
  6. the survivors are appended to M in rank order.
A radius: passes until one appends nothing, or ``max_passes`` of them.  "passes"
counts every pass that ran, the last, empty one included; "triangles" and
"dropped" have an entry per pass that ran.  "converged": every radius ended
with an empty pass.

Two forms are carried: ``candidates`` (per query i, over i's 2r-neighbourhood)
and ``candidates_brute`` (the definition: all triples, every blocker named by
the rule found by a scan of the whole cloud, no grid, no tree).

Solving every case below takes 20 s on one core of the development machine
(measured with ``python -m tests.bpa_oracle``).
"""
import itertools
import time

import numpy as np
from scipy.spatial import cKDTree

ORPHAN, BORDER, INNER = 0, 1, 2


def _d2(u, v):
    d = u - v
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _geometry(p0, p1, p2, n0, n1, n2, r2):
    """The circumcentre, normal and ball-centre rules for arrays of triples ->
    (ok bool [m], sign f64 [m], o f64 [m, 3]); the neighbour tests are the caller's."""
    with np.errstate(all="ignore"):
        a, b, c = _d2(p1, p2), _d2(p2, p0), _d2(p0, p1)
        wa = a * ((b + c) - a)
        wb = b * ((a + c) - b)
        wc = c * ((a + b) - c)
        s = (wa + wb) + wc
        ok = s > 0
        cc = (p0 * (wa / s)[:, None] + p1 * (wb / s)[:, None]) + p2 * (wc / s)[:, None]
        h = r2 - _d2(cc, p0)
        ok &= h >= 0
        e1, e2 = p1 - p0, p2 - p0
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        ok &= ln > 0
        d = [(n[:, 0] * m[:, 0] + n[:, 1] * m[:, 1]) + n[:, 2] * m[:, 2] for m in (n0, n1, n2)]
        pos = (d[0] > 0) & (d[1] > 0) & (d[2] > 0)
        neg = (d[0] < 0) & (d[1] < 0) & (d[2] < 0)
        ok &= pos | neg
        sign = np.where(neg, -1.0, 1.0)
        o = cc + (n / ln[:, None]) * (sign * np.sqrt(h))[:, None]
    return ok, sign, o


def _wound(i, j, k, sign):
    neg = sign < 0
    return np.stack([i, np.where(neg, k, j), np.where(neg, j, k)], 1).astype(np.int32).reshape(-1, 3)


def _neighbourhoods(P, r):
    """Per point, the indices q with d2(q, p) < R4 (ascending; the point itself included)."""
    R4 = 4.0 * (r * r)
    n = len(P)
    if n == 0:
        return []
    if n <= 2048:
        out = []
        for i in range(n):
            out.append(np.nonzero(_d2(P, P[i]) < R4)[0])
        return out
    lists = cKDTree(P).query_ball_point(P, 2.0 * r * (1.0 + 1e-9) + 1e-300)
    out = []
    for i, c in enumerate(lists):
        c = np.sort(np.asarray(c, dtype=np.int64))
        out.append(c[_d2(P[c], P[i]) < R4])
    return out


def candidates(P, N, r, vclass=None, nbs=None):
    """-> int32 [C, 3], wound, in rank order: the candidate triangles at radius
    r whose vertices are all non-inner (``vclass`` None: every point an orphan)."""
    P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 3)
    N = np.ascontiguousarray(N, dtype=np.float64).reshape(-1, 3)
    n = len(P)
    r = float(r)
    r2 = r * r
    R4 = 4.0 * r2
    live = np.ones(n, dtype=bool) if vclass is None else np.asarray(vclass) != INNER
    nbs = _neighbourhoods(P, r) if nbs is None else nbs
    out = []
    for i in np.nonzero(live)[0]:
        nb = nbs[i]
        el = nb[(nb > i) & live[nb]]
        if len(el) < 2:
            continue
        a, b = np.triu_indices(len(el), 1)
        j, k = el[a], el[b]  # el ascends: j < k
        near = _d2(P[j], P[k]) < R4
        j, k = j[near], k[near]
        if not len(j):
            continue
        ii = np.full(len(j), i)
        ok, sign, o = _geometry(P[ii], P[j], P[k], N[ii], N[j], N[k], r2)
        j, k, sign, o = j[ok], k[ok], sign[ok], o[ok]
        # emptiness over i's 2r-neighbourhood, a slice of blockers at a time
        alive = np.arange(len(j))
        c1, step = 0, 8  # (no point is inside: the order and the slicing of the blockers do not matter)
        while c1 < len(nb) and len(alive):
            c0, c1, step = c1, c1 + step, 4 * step
            q = nb[c0:c1]
            with np.errstate(all="ignore"):
                inside = _d2(P[q][None, :, :], o[alive][:, None, :]) < r2
            inside &= (q[None, :] != i) & (q[None, :] != j[alive][:, None]) & (q[None, :] != k[alive][:, None])
            alive = alive[~inside.any(1)]
        if len(alive):
            out.append(_wound(np.full(len(alive), i), j[alive], k[alive], sign[alive]))  # (j, k) ascend
    return np.concatenate(out) if out else np.zeros((0, 3), np.int32)


def candidates_brute(P, N, r, vclass=None):
    """The definition: every triple i < j < k, every point of the cloud scanned for the blockers."""
    P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 3)
    N = np.ascontiguousarray(N, dtype=np.float64).reshape(-1, 3)
    n = len(P)
    r2 = float(r) * float(r)
    R4 = 4.0 * r2
    live = np.ones(n, dtype=bool) if vclass is None else np.asarray(vclass) != INNER
    out = []
    for i, j, k in itertools.combinations(range(n), 3):
        if not (live[i] and live[j] and live[k]):
            continue
        p0, p1, p2 = P[i], P[j], P[k]
        if not (_d2(p1, p0) < R4 and _d2(p2, p0) < R4 and _d2(p1, p2) < R4):
            continue
        ok, sign, o = _geometry(p0[None], p1[None], p2[None], N[i][None], N[j][None], N[k][None], r2)
        if not ok[0]:
            continue
        with np.errstate(all="ignore"):
            block = (_d2(P, p0) < R4) & (_d2(P, o[0]) < r2)
        block[[i, j, k]] = False
        if not block.any():
            out.append((i, k, j) if sign[0] < 0 else (i, j, k))
    return np.asarray(out, dtype=np.int32).reshape(-1, 3)


def _edge_keys(T, n):
    """int64 [t, 3]: the keys a n + b (a < b) of the edges (v0 v1, v1 v2, v2 v0) of the sorted triples."""
    S = np.sort(T.astype(np.int64), 1)
    return np.stack([S[:, 0] * n + S[:, 1], S[:, 1] * n + S[:, 2], S[:, 0] * n + S[:, 2]], 1)


def _count_in(sorted_keys, keys):
    return np.searchsorted(sorted_keys, keys, "right") - np.searchsorted(sorted_keys, keys, "left")


def vertex_classes(T, n):
    cls = np.zeros(n, dtype=np.uint8)
    if len(T):
        cls[T.reshape(-1)] = INNER
        keys = np.sort(_edge_keys(T, n).reshape(-1))
        once = keys[_count_in(keys, keys) == 1]
        cls[once // n] = BORDER
        cls[once % n] = BORDER
    return cls


def border_edges(T, n):
    if not len(T):
        return 0
    keys = np.sort(_edge_keys(T, n).reshape(-1))
    return int((_count_in(keys, keys) == 1).sum())


def one_pass(P, N, r, T, nbs=None, C=None):
    """Rules 1-6 -> (the appended triangles int32 [t, 3] in rank order, the number rule 5 dropped).
    ``C``: the candidates of rule 1, when the caller has them already."""
    n = len(P)
    cls = vertex_classes(T, n)
    if C is None:
        C = candidates(P, N, r, cls if len(T) else None, nbs)
    if not len(C):
        return C, 0
    S = np.sort(C.astype(np.int64), 1)
    ek = _edge_keys(C, n)
    mk = np.sort(_edge_keys(T, n).reshape(-1)) if len(T) else np.zeros(0, np.int64)
    cm = _count_in(mk, ek)  # [c, 3]
    keep = np.ones(len(C), dtype=bool)
    if len(T):  # rule 2
        have = {tuple(t) for t in np.sort(T.astype(np.int64), 1).tolist()}
        keep &= np.array([tuple(t) not in have for t in S.tolist()])
    keep &= (cm < 2).all(1)  # rule 3
    orphans = (cls[S] == ORPHAN).all(1)
    keep &= (cm > 0).any(1) | orphans  # rule 4
    idx = np.nonzero(keep)[0]  # rank order
    flat_key = ek[idx].reshape(-1)
    flat_tri = np.repeat(np.arange(len(idx)), 3)
    order = np.argsort(flat_key, kind="stable")  # by key, then by rank
    sk = flat_key[order]
    place = np.arange(len(sk)) - np.searchsorted(sk, sk, "left")
    bad = place >= 2 - _count_in(mk, sk)
    dropped = np.zeros(len(idx), dtype=bool)
    dropped[flat_tri[order][bad]] = True
    return C[idx[~dropped]], int(dropped.sum())


def ball_pivoting(P, N, radii, max_passes=8, first=None):
    """-> (triangles int32 [T, 3] in pass order, then rank order; info).  ``first``: the candidates
    of the first radius on the all-orphan cloud, when the caller has them already."""
    P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 3)
    N = np.ascontiguousarray(N, dtype=np.float64).reshape(-1, 3)
    T = np.zeros((0, 3), np.int32)
    info = {"passes": [], "triangles": [], "dropped": [], "border_edges": 0, "converged": True}
    for r in radii:
        nbs = _neighbourhoods(P, float(r))
        done = False
        passes = 0
        while passes < max_passes and not done:
            new, dropped = one_pass(P, N, float(r), T, nbs, first if not info["triangles"] else None)
            passes += 1
            info["triangles"].append(len(new))
            info["dropped"].append(dropped)
            T = np.concatenate([T, new])
            done = len(new) == 0
        info["passes"].append(passes)
        info["converged"] = info["converged"] and done
    info["border_edges"] = border_edges(T, len(P))
    return T, info


# ------------------------------------------------------------------ cases ----
def mean_nn(P):
    d = cKDTree(P).query(P, k=2)[0][:, 1]
    return float(d.mean())


def _up(n):
    return np.tile([[0.0, 0.0, 1.0]], (n, 1))


def _sheet(rng, nx, ny, jitter, z_noise):
    g = np.stack(np.meshgrid(np.arange(float(nx)), np.arange(float(ny)), indexing="ij"), -1).reshape(-1, 2)
    g = g + rng.uniform(-jitter, jitter, g.shape)
    return np.concatenate([g, rng.normal(size=(len(g), 1)) * z_noise], 1)


def case_empty():
    return np.zeros((0, 3)), np.zeros((0, 3)), [1.0]


def case_one_point():
    return np.array([[1.0, 2.0, 3.0]]), _up(1), [1.0]


def case_two_points():
    return np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]]), _up(2), [1.0]


_TRI = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.3, 0.9, 0.0]])  # circumradius 0.6009


def case_triangle_above():
    return _TRI, _up(3), [0.61]


def case_triangle_below():
    return _TRI, _up(3), [0.59]


_STRICT = np.array([[-1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


def case_strict_closed():  # the pair at distance exactly 2 r is no neighbour
    return _STRICT, _up(3), [1.0]


def case_strict_open():
    return _STRICT, _up(3), [float(np.nextafter(1.0, 2.0))]


def patch():
    """A flat jittered patch: the balls on its two sides are mirror images, exactly."""
    P = _sheet(np.random.default_rng(11), 8, 8, 0.25, 0.0)
    return P, _up(len(P)), [0.9]


def case_patch():
    return patch()


def case_patch_flipped():
    P, N, radii = patch()
    return P, -N, radii


PATCH_ODD_VERTEX = 27


def case_patch_one_incompatible():
    P, N, radii = patch()
    N = N.copy()
    N[PATCH_ODD_VERTEX] = -N[PATCH_ODD_VERTEX]
    return P, N, radii


def sphere(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v


def case_sphere_1500():
    P = sphere(1500, 1)
    d = mean_nn(P)
    return P, P.copy(), [d, 2 * d, 4 * d]


def case_shuffled():
    """A wavy sheet over several thousand grid cells, its index order a random permutation of its
    spatial order."""
    rng = np.random.default_rng(12)
    P = _sheet(rng, 60, 60, 0.3, 0.0)
    P[:, 2] = 0.8 * np.sin(P[:, 0] / 5.0) * np.cos(P[:, 1] / 7.0)
    N = np.stack([-0.16 * np.cos(P[:, 0] / 5.0) * np.cos(P[:, 1] / 7.0),
                  0.8 / 7.0 * np.sin(P[:, 0] / 5.0) * np.sin(P[:, 1] / 7.0), np.ones(len(P))], 1)
    perm = rng.permutation(len(P))
    return P[perm], N[perm], [0.5, 1.0]  # cells of edge 1: 60 x 60 of them


def case_single_cell():
    """A cloud inside one grid cell: its extent is below the cell edge 2 r."""
    P = _sheet(np.random.default_rng(13), 7, 7, 0.3, 0.1) * 0.1
    P = P[np.random.default_rng(14).permutation(len(P))]
    return P, _up(len(P)), [0.5]


def case_two_sheets():
    """Two parallel jittered sheets 0.9 apart (closer than 2 r = 1.6), the normals facing away from
    each other: blockers and incompatible triples from the other sheet."""
    rng = np.random.default_rng(15)
    A = _sheet(rng, 14, 14, 0.25, 0.03)
    B = _sheet(rng, 14, 14, 0.25, 0.03)
    B[:, 2] -= 0.9
    P = np.concatenate([A, B])
    N = np.concatenate([_up(len(A)), -_up(len(B))])
    perm = rng.permutation(len(P))
    return P[perm], N[perm], [0.8, 1.6]


def case_lattice():
    g = np.stack(np.meshgrid(np.arange(9.0), np.arange(8.0), indexing="ij"), -1).reshape(-1, 2)
    P = np.concatenate([g, np.zeros((len(g), 1))], 1)
    P = P[np.random.default_rng(16).permutation(len(P))]
    return P, _up(len(P)), [0.75, 1.5]


def case_duplicates():
    rng = np.random.default_rng(17)
    P = _sheet(rng, 10, 10, 0.25, 0.05)
    P = np.concatenate([P, P[:12], P[5:8]])  # doubled and tripled points: s = 0 triples, zero distances
    perm = rng.permutation(len(P))
    return P[perm], _up(len(P)), [0.9, 1.8]


def case_dense_blob():
    """400 points in a ball of diameter 1.9 r: every neighbourhood holds all of them (seven staging
    tiles of 64), normals radial."""
    rng = np.random.default_rng(18)
    v = rng.normal(size=(400, 3))
    v *= (0.95 * rng.uniform(0.0, 1.0, (400, 1)) ** (1.0 / 3.0)) / np.linalg.norm(v, axis=1, keepdims=True)
    return v + np.array([5.0, -3.0, 2.0]), v.copy(), [1.0]


def case_hole_fill():
    """A jittered sheet without the points within 1.6 of its centre: at the first radius the hole
    stays open (a ring of a dozen border edges); the second radius closes it from the rim inwards."""
    P = _sheet(np.random.default_rng(19), 13, 13, 0.2, 0.02)
    P = P[np.hypot(P[:, 0] - 6.0, P[:, 1] - 6.0) > 1.6]
    return P, _up(len(P)), [0.8, 2.4]


def case_jittered_grid():
    """38 x 38 points, z noise of 0.15 grid spacings, multipliers 1, 2, 4: rule 5 drops triangles."""
    P = _sheet(np.random.default_rng(20), 38, 38, 0.3, 0.15)
    d = mean_nn(P)
    return P, _up(len(P)), [d, 2 * d, 4 * d]


CASES = {
    "empty": case_empty,
    "one_point": case_one_point,
    "two_points": case_two_points,
    "triangle_above": case_triangle_above,
    "triangle_below": case_triangle_below,
    "strict_closed": case_strict_closed,
    "strict_open": case_strict_open,
    "patch": case_patch,
    "patch_flipped": case_patch_flipped,
    "patch_one_incompatible": case_patch_one_incompatible,
    "sphere_1500": case_sphere_1500,
    "shuffled": case_shuffled,
    "single_cell": case_single_cell,
    "two_sheets": case_two_sheets,
    "lattice": case_lattice,
    "duplicates": case_duplicates,
    "dense_blob": case_dense_blob,
    "hole_fill": case_hole_fill,
    "jittered_grid": case_jittered_grid,
}

_solved = {}


def solved(name):
    """The case and its oracle results, computed once per process: {"P", "N", "radii", "candidates"
    (per radius, on the all-orphan cloud), "T", "info"}."""
    if name not in _solved:
        P, N, radii = CASES[name]()
        cands = [candidates(P, N, r) for r in radii]
        T, info = ball_pivoting(P, N, radii, first=cands[0])
        for a in (T, *cands):  # shared among the tests: not to be changed
            a.setflags(write=False)
        _solved[name] = {"P": P, "N": N, "radii": list(radii), "candidates": cands, "T": T, "info": info}
    return _solved[name]


if __name__ == "__main__":
    t_all = time.perf_counter()
    for name in CASES:
        t0 = time.perf_counter()
        s = solved(name)
        print(f"{name:24s} n={len(s['P']):5d} T={len(s['T']):5d} cand={[len(c) for c in s['candidates']]} "
              f"{s['info']}  {time.perf_counter() - t0:.2f} s")
    print(f"all cases: {time.perf_counter() - t_all:.1f} s")
