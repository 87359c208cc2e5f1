"""Named inputs of the mesh smoothing tests (tests/test_meshsmooth_oracle.py on the CPU,
tests/test_gpu_meshsmooth.py on the GPU): the smallest shapes at which the kernels of
csrc/slmeshsmooth.inl can go wrong -- rows around the wave (64), the workgroup (256) and the sort
tile (4096), empty first and last rows, keys beyond 32 and 40 bits, repeated indices."""
from __future__ import annotations

import functools

import numpy as np

from tests import meshclean_cases as mc
from tests import meshsmooth_oracle as so

I32 = np.int32
_t = mc._t
BAD_INDEX_CASES = mc.BAD_INDEX_CASES

HUB_DEGREES = (63, 64, 65, 255, 256, 257, 4097)
STRIP_SIZES = (255, 256, 257, 4095, 4096, 4097)
RANDOM_V = (15, 16, 17, 255, 256, 257, 65537, 1048577)


def hub_fan(degree, seed):
    """An open fan of degree - 1 triangles about a hub with `degree` rim vertices (the hub's row has `degree`
    entries, the rim's two or three), the numbering shuffled -> (triangles, n_vertices, the hub's index)."""
    perm = np.random.default_rng(seed).permutation(degree + 1)
    i = np.arange(degree - 1)
    T = np.stack([np.zeros_like(i), 1 + i, 2 + i], 1)
    return perm[T].astype(I32), degree + 1, int(perm[0])


def grid_sheet(nx, ny, seed):
    """An open nx x ny sheet of vertices, two triangles a cell, the numbering shuffled: interior vertices of degree
    6 and a boundary ring -> (triangles, n_vertices)."""
    perm = np.random.default_rng(seed).permutation(nx * ny)
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="ij")
    a = (i * ny + j).ravel()
    T = np.concatenate([np.stack([a, a + ny, a + 1], 1), np.stack([a + 1, a + ny, a + ny + 1], 1)])
    return perm[T].astype(I32), nx * ny


def adjacency_cases():
    """name -> (triangles int32 [T, 3], n_vertices)."""
    c = {}
    c["none"] = (_t([]), 5)
    c["nothing"] = (_t([]), 0)
    c["one"] = (_t([[0, 1, 2]]), 3)
    c["shared_edge"] = (_t([[0, 1, 2], [2, 1, 3]]), 4)
    c["same_twice"] = (_t([[0, 1, 2], [0, 1, 2]]), 3)
    c["opposite_windings"] = (_t([[0, 1, 2], [0, 2, 1]]), 3)
    c["aab"] = (_t([[0, 0, 1]]), 2)
    c["aaa"] = (_t([[2, 2, 2]]), 4)
    c["repeats_mixed"] = (_t([[0, 0, 1], [1, 0, 2], [3, 3, 4], [5, 5, 5], [5, 5, 6], [7, 8, 9], [4, 3, 3]]), 10)
    c["empty_first_and_last_rows"] = (_t([[1, 2, 3], [3, 2, 4], [6, 6, 7]]), 9)   # 0, 5 and 8 are of no triangle
    for d in HUB_DEGREES:
        c[f"hub_{d}"] = hub_fan(d, d)[:2]
    for n in STRIP_SIZES:
        c[f"strip_{n}"] = mc.strip(n, 7 * n)
    for v in RANDOM_V:
        c[f"v_{v}"] = mc.random_triples(v, 40, v)   # the top indices: keys beyond 32 bits at 65537, 40 at 1048577
    c["sheet_9x7"] = grid_sheet(9, 7, 2)
    c["sphere"] = (sphere()[1], 362)
    return c


def sphere():
    """The lat-long unit sphere: 15 rings x 24 meridians plus the poles, 362 vertices, 720 triangles, closed."""
    rings, mer = 15, 24
    th = np.pi * (np.arange(rings) + 1) / (rings + 1)
    ph = 2.0 * np.pi * np.arange(mer) / mer
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)),
                     np.outer(np.cos(th), np.ones(mer))], -1).reshape(-1, 3)
    P = np.concatenate([[[0.0, 0.0, 1.0]], ring, [[0.0, 0.0, -1.0]]])
    at = lambda r, m: 1 + r * mer + (m % mer)  # noqa: E731
    T = []
    for m in range(mer):
        T.append([0, at(0, m), at(0, m + 1)])
        for r in range(rings - 1):
            T.append([at(r, m), at(r + 1, m), at(r + 1, m + 1)])
            T.append([at(r, m), at(r + 1, m + 1), at(r, m + 1)])
        T.append([len(P) - 1, at(rings - 1, m + 1), at(rings - 1, m)])
    return P, _t(T)


def noisy_sphere():
    """``sphere`` with every radius multiplied by 1 + 0.02 default_rng(1).standard_normal -> (vertices, triangles)."""
    P, T = sphere()
    return P * (1.0 + 0.02 * np.random.default_rng(1).standard_normal(len(P)))[:, None], T


def spoke_fan(seed=4):
    """A hub fan of 65 spokes whose lengths span 10^-6 .. 10^6, shuffled in index: the weights of one row span
    twelve decades, so the order of the fold shows in the last bits -> (vertices, triangles, the hub)."""
    T, nv, hub = hub_fan(65, seed)
    rng = np.random.default_rng(seed)
    P = np.zeros((nv, 3))
    P[hub] = (0.3, -0.2, 0.1)
    rim = np.array([v for v in range(nv) if v != hub])
    length = 10.0 ** rng.uniform(-6.0, 6.0, size=len(rim))
    u = rng.normal(size=(len(rim), 3))
    P[rim] = P[hub] + length[:, None] * u / np.linalg.norm(u, axis=1)[:, None]
    return P, T, hub


def _normal(nv, seed):
    return np.random.default_rng(seed).normal(size=(nv, 3))


def filter_meshes():
    """name -> (vertices f64 [V, 3], triangles int32 [T, 3])."""
    c = {}
    for n in STRIP_SIZES:
        T, nv = mc.strip(n, 7 * n)
        c[f"strip_{n}"] = (_normal(nv, n), T)
    for d in HUB_DEGREES:
        T, nv, _ = hub_fan(d, d)
        c[f"hub_{d}"] = (_normal(nv, d), T)
    c["spoke_fan"] = spoke_fan()[:2]
    P = _normal(6, 1)
    P[3] = P[1]                                                        # dist 0: weight 10^12
    c["coincident"] = (P, _t([[0, 1, 3], [1, 2, 3], [3, 4, 5]]))
    # 6 is in (6, 6, 6) alone: N(6) = {6}; 7 and 0 are of no triangle
    c["isolated_and_unreferenced"] = (_normal(8, 2), _t([[1, 2, 3], [3, 2, 4], [6, 6, 6], [4, 5, 1]]))
    c["degenerate"] = (_normal(7, 3), _t([[0, 0, 1], [1, 0, 2], [3, 3, 4], [5, 5, 6], [2, 4, 6], [4, 3, 3]]))
    T, nv = grid_sheet(9, 7, 2)
    c["sheet_9x7"] = (_normal(nv, 5), T)
    c["noisy_sphere"] = noisy_sphere()
    c["no_triangles"] = (_normal(5, 6), _t([]))
    c["nothing"] = (np.zeros((0, 3)), _t([]))
    return c


def _runs():
    """id -> (mesh name, method, keywords): every call the CPU and the GPU suites check."""
    r = {}

    def add(mesh, method, **kw):
        tag = "-".join(f"{k}={v}" for k, v in kw.items())
        r[f"{mesh}-{method}" + (f"-{tag}" if tag else "")] = (mesh, method, kw)

    for name in [f"strip_{n}" for n in STRIP_SIZES] + [f"hub_{d}" for d in HUB_DEGREES]:
        add(name, "simple")
        add(name, "laplacian")
        add(name, "taubin", iterations=2)
    for lam in (0.5, 1.0, -0.25):
        add("spoke_fan", "laplacian", lambda_filter=lam)
        add("sheet_9x7", "laplacian", iterations=2, lambda_filter=lam)
        add("sheet_9x7", "taubin", iterations=2, lambda_filter=lam, mu=-0.53)
    add("spoke_fan", "simple", iterations=2)
    add("spoke_fan", "taubin", iterations=10)
    for name in ("coincident", "isolated_and_unreferenced", "degenerate", "no_triangles", "nothing"):
        add(name, "simple", iterations=2)
        add(name, "laplacian", iterations=2)
        add(name, "taubin", iterations=1)
    for method in ("simple", "laplacian", "taubin"):
        add("strip_257", method, iterations=2, fixed_boundary=True)      # every vertex of a strip is boundary
        add("sheet_9x7", method, iterations=2, fixed_boundary=True)      # the ring stays, the interior moves
        add("noisy_sphere", method, iterations=2, fixed_boundary=True)   # closed: nothing is fixed
        for it in (0, 1, 2, 10):
            add("noisy_sphere", method, iterations=it)
    return r


RUNS = _runs()
MESHES = filter_meshes()


@functools.lru_cache(maxsize=None)
def reference(run):
    """The order-free oracle's result of RUNS[run], computed once per process (read-only)."""
    mesh, method, kw = RUNS[run]
    P, T = MESHES[mesh]
    out = so.FILTERS[method](P, T, **kw)
    out.setflags(write=False)
    return out
