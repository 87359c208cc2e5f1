"""Named inputs of the mesh check tests (tests/test_meshcheck_oracle.py on the CPU, tests/test_gpu_meshcheck.py on
the GPU): the smallest shapes at which the kernels of csrc/slmeshcheck.inl can go wrong -- runs of sides around the
wave (64), the workgroup (256) and the sort tile (4096), long parity chains, corner classes of one vertex, keys
beyond 32 and 40 bits, degenerate and repeated triangles, surfaces that are closed but not orientable."""
from __future__ import annotations

import functools

import numpy as np

from tests import meshclean_cases as mc
from tests import meshsmooth_cases as sm

I32 = np.int32
_t = mc._t
BAD_INDEX_CASES = mc.BAD_INDEX_CASES

BOOK_PAGES = (3, 63, 64, 65, 257, 4097)
MOBIUS_QUADS = (5, 255, 257, 4097)
RANDOM_V = sm.RANDOM_V


def _quads(a, b, c, d):
    """Two triangles per quad a-b-c-d (a -> b -> c -> d around it)."""
    return np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(I32)


def tetrahedron():
    """Volume 1/6, wound outward."""
    P = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    return P, _t([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])


def cube():
    """The integer unit cube, 12 triangles wound outward: area 6.0, volume 1.0."""
    P = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])   # index 4 x + 2 y + z
    q = np.array([[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]])
    return P, _quads(q[:, 0], q[:, 1], q[:, 2], q[:, 3])


def grid_surface(nu, nv, klein=False):
    """A closed nu x nv grid of quads on a torus' positions; ``klein``: the u seam is glued with v reversed (a Klein
    bottle: closed, edge- and vertex-manifold, not orientable) -> (vertices, triangles)."""
    u, v = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    th, ph = 2.0 * np.pi * u / nu, 2.0 * np.pi * v / nv
    P = np.stack([(2.0 + 0.5 * np.cos(ph)) * np.cos(th), (2.0 + 0.5 * np.cos(ph)) * np.sin(th), 0.5 * np.sin(ph)],
                 -1).reshape(-1, 3)

    def at(i, j):
        wrap = i >= nu
        j = np.where(wrap & klein, -j, j) % nv
        return (i % nu) * nv + j
    i, j = u.ravel(), v.ravel()
    return P, _quads(at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1))


def mobius(n):
    """A strip of n quads whose ends are glued with a half twist: edge- and vertex-manifold, one boundary loop, not
    orientable -> (triangles, n_vertices)."""
    i = np.arange(n)
    lo, hi = i, n + i
    nlo = np.where(i + 1 < n, i + 1, n)          # the last quad meets column 0 with the rows swapped
    nhi = np.where(i + 1 < n, n + i + 1, 0)
    return _quads(lo, nlo, nhi, hi), 2 * n


def book(m):
    """m triangles on one spine edge: one run of m sides -> (triangles, n_vertices)."""
    i = np.arange(m)
    return np.stack([np.zeros_like(i), np.ones_like(i), 2 + i], 1).astype(I32), m + 2


def cone(degree, seed):
    """``meshsmooth_cases.hub_fan`` closed around the hub: `degree` triangles, the hub's corners one class."""
    T, nv, hub = sm.hub_fan(degree, seed)
    first, last = T[0, 1], T[-1, 2]
    return np.concatenate([T, _t([[hub, last, first]])]), nv


def fans_at_hub(k):
    """k fans of two triangles each that share only the hub: its corners fall into k classes."""
    i = np.arange(k)
    return np.concatenate([np.stack([np.zeros_like(i), 1 + 3 * i, 2 + 3 * i], 1),
                           np.stack([np.zeros_like(i), 2 + 3 * i, 3 + 3 * i], 1)]).astype(I32), 3 * k + 1


def _glue(T, offset, shared):
    """A copy of T on new vertices, except that the vertices in ``shared`` stay."""
    m = np.arange(int(T.max()) + 1) + offset
    for s in shared:
        m[s] = s
    return m[T].astype(I32)


def flipped(T, seed=None):
    """Every triangle (seed None) or a seeded random half as (a, c, b)."""
    T = np.asarray(T, dtype=I32).reshape(-1, 3)
    pick = np.ones(len(T), dtype=bool) if seed is None else np.random.default_rng(seed).random(len(T)) < 0.5
    out = T.copy()
    out[pick] = T[pick][:, [0, 2, 1]]
    return out


def shuffled(P, T, nv, seed):
    """The same mesh in another vertex and triangle numbering."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(nv)
    Tn = perm[np.asarray(T, dtype=np.int64).reshape(-1, 3)][rng.permutation(len(T))].astype(I32).reshape(-1, 3)
    Pn = None
    if P is not None:
        Pn = np.empty_like(P)
        Pn[perm] = P
    return Pn, Tn, nv


def closed_meshes():
    """name -> (vertices, triangles): closed, orientable, wound outward."""
    c = {"tetrahedron": tetrahedron(), "cube": cube(), "sphere": sm.sphere(), "torus_64x65": grid_surface(64, 65),
         "torus_3x1366": grid_surface(3, 1366)}
    return c


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (vertices f64 [V, 3] | None, triangles int32 [T, 3], n_vertices)."""
    c = {}
    adj = sm.adjacency_cases()
    for name in ("none", "nothing", "one", "shared_edge", "same_twice", "opposite_windings", "aab", "aaa",
                 "repeats_mixed", "empty_first_and_last_rows", "sheet_9x7"):
        c[name] = (None, *adj[name])
    # a degenerate triangle between two others in one run: the corner chain has to pass over it
    c["degenerate_in_run"] = (None, _t([[0, 1, 2], [0, 1, 0], [1, 0, 3], [4, 4, 5], [5, 4, 6]]), 7)
    for name, (P, T) in closed_meshes().items():
        c[name] = (P, T, len(P))
        c[name + "_half_flipped"] = (P, flipped(T, seed=len(T)), len(P))
        c[name + "_all_flipped"] = (P, flipped(T), len(P))
    for n in (255, 257, 4097):
        c[f"strip_{n}"] = (None, *mc.strip(n, 3 * n))
    for m in BOOK_PAGES:
        c[f"book_{m}"] = (None, *book(m))
    for d in sm.HUB_DEGREES:
        c[f"fan_{d}"] = (None, *sm.hub_fan(d, d)[:2])
        c[f"cone_{d}"] = (None, *cone(d, d))
    P, T = tetrahedron()
    c["two_tetrahedra_one_vertex"] = (None, np.concatenate([T, _glue(T, 4, (0,))]), 8)
    c["two_tetrahedra_one_edge"] = (None, np.concatenate([T, _glue(T, 4, (0, 1))]), 8)
    T, nv = cone(12, 1)
    hub = int(T[0, 0])
    c["two_cones_one_apex"] = (None, np.concatenate([T, _glue(T, nv, (hub,))]), 2 * nv)
    c["fans_65_at_hub"] = (None, *fans_at_hub(65))
    for n in MOBIUS_QUADS:
        c[f"mobius_{n}"] = (None, *mobius(n))
    P, T = grid_surface(8, 9, klein=True)
    c["klein_8x9"] = (P, T, len(P))
    for v in RANDOM_V:
        c[f"v_{v}"] = (None, *mc.random_triples(v, 40, v))
    tiny = {"none", "nothing", "one", "shared_edge", "same_twice", "opposite_windings", "aab", "aaa", "repeats_mixed",
            "empty_first_and_last_rows", "degenerate_in_run"}
    for name in [n for n in c if n not in tiny and not n.startswith("v_")]:     # every structured case
        P, T, nv = c[name]
        c[name + "_shuffled"] = shuffled(P, T, nv, seed=len(T) + 1)
    return c


STRUCTURED_SHUFFLED = tuple(n[: -len("_shuffled")] for n in cases() if n.endswith("_shuffled"))


@functools.lru_cache(maxsize=None)
def reference(name, what):
    """The oracle's result on cases()[name], computed once per process.  what: "check", "edges" (allowed boundary),
    "edges_closed", "vertices", "orient", "degenerate", "duplicated"."""
    from tests import meshcheck_oracle as ko
    P, T, nv = cases()[name]
    if what == "check":
        return ko.check(P, T, nv)
    if what == "edges":
        return ko.get_non_manifold_edges(T, nv, True)
    if what == "edges_closed":
        return ko.get_non_manifold_edges(T, nv, False)
    if what == "vertices":
        return ko.get_non_manifold_vertices(T, nv)
    if what == "orient":
        return ko.orient_triangles(T, nv)
    if what == "degenerate":
        return ko.remove_degenerate_triangles(T, nv)
    if what == "duplicated":
        return ko.remove_duplicated_triangles(T, nv)
    raise KeyError(what)
