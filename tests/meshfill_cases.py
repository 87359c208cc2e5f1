"""Named inputs of the hole-filling tests (tests/test_meshfill_oracle.py on the CPU, tests/test_gpu_meshfill.py on the
GPU): the smallest shapes at which the rules of csrc/slmeshfill.inl can go wrong -- loops of three and four sides,
two loops whose labels come in either order, holes that touch, fans at a non-manifold vertex, self-loops of
degenerate triangles, loops longer than a wave and than a workgroup, vertices far from the origin and on one axis."""
from __future__ import annotations

import functools

import numpy as np

from tests import meshcheck_cases as kc
from tests import meshclean_cases as mc

I32 = np.int32
_t = mc._t


def _positions(nv, seed):
    return np.random.default_rng(seed).normal(size=(nv, 3))


def sheet(nx, ny, holes=()):
    """A flat nx x ny sheet of quads in z = 0 without the quads (i, j) in ``holes`` -> (vertices, triangles)."""
    x, y = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    P = np.stack([x.ravel(), y.ravel(), np.zeros(x.size)], 1).astype(np.float64)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    keep = np.ones((nx, ny), dtype=bool)
    for h in holes:
        keep[h] = False
    i, j = i[keep], j[keep]

    def at(a, b):
        return a * (ny + 1) + b
    return P, kc._quads(at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1))


def open_cylinder(nu, nv):
    """``meshcheck_cases.grid_surface`` (a torus) without its last ring of quads and without the first triangle of
    every quad of the ring before it: an open cylinder with a straight rim of nv sides and a zigzag rim of 2 nv
    -> (vertices, triangles)."""
    P, T = kc.grid_surface(nu, nv)
    q = nu * nv                                    # rows 0 .. q - 1: (a, b, c) of quad i nv + j; q .. 2 q - 1: (a, c, d)
    ring = np.arange(q) // nv
    keep = np.concatenate([ring < nu - 2, ring < nu - 1])
    return P, T[keep]


def cone_mesh(degree, seed):
    """``meshcheck_cases.cone`` with positions: the hub above a circle -> (vertices, triangles)."""
    T, nv = kc.cone(degree, seed)
    hub = int(T[0, 0])
    P = np.zeros((nv, 3))
    rim = T[:, 1]                                  # every rim vertex is the second corner of one triangle
    th = 2.0 * np.pi * np.arange(degree) / degree
    P[rim] = np.stack([np.cos(th), np.sin(th), np.zeros(degree)], 1)
    P[hub] = (0.0, 0.0, 1.0)
    return P, T


def without_rows(P, T, rows):
    return P, np.delete(T, rows, axis=0)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (vertices f64 [V, 3], triangles int32 [T, 3])."""
    c = {}
    K = kc.cases()

    def shuffled(name, seed):
        P, T = c[name]
        Pn, Tn, _ = kc.shuffled(P, T, len(P), seed)
        c[f"{name}_shuffled_{seed}"] = (Pn, Tn)
    c["empty"] = (np.zeros((0, 3)), _t([]))
    c["vertices_only"] = (_positions(5, 0), _t([]))
    c["single_triangle"] = (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), _t([[0, 1, 2]]))
    c["tetrahedron_minus_face"] = without_rows(*kc.tetrahedron(), [3])
    c["tetrahedron_minus_first_face"] = without_rows(*kc.tetrahedron(), [0])
    c["cube_minus_face"] = without_rows(*kc.cube(), [1, 7])           # the face x = 1: centre (1, 0.5, 0.5)
    for name in ("tetrahedron", "cube", "torus_64x65", "klein_8x9"):    # no boundary
        c[name] = K[name][:2]
    c["cylinder"] = open_cylinder(5, 7)                                 # loops of 7 and 14 sides
    shuffled("cylinder", 1)
    shuffled("cylinder", 2)
    # two holes that touch in vertex (2, 2), a hole of its own, and the outer rim
    c["figure_eight"] = sheet(6, 5, holes=((1, 1), (2, 2), (4, 3)))
    shuffled("figure_eight", 3)
    for name in ("two_cones_one_apex", "fans_65_at_hub", "degenerate_in_run", "book_3", "book_65", "aab", "aaa",
                 "repeats_mixed", "mobius_5", "mobius_257", "strip_257", "sheet_9x7", "fan_65"):
        _, T, nv = K[name]
        c[name] = (_positions(nv, len(T)), T)
    shuffled("two_cones_one_apex", 4)
    for d in (65, 129, 5000):                                            # more than a wave, a workgroup, one long loop
        c[f"cone_{d}"] = cone_mesh(d, d)
    P, T = c["cone_65"]
    P2, T2 = c["cone_129"]
    c["cones_65_129"] = (np.concatenate([P, P2 + np.array([3.0, 0.0, 0.0])]), np.concatenate([T, T2 + len(P)]))
    shuffled("cones_65_129", 5)
    # the fixed-point scale: far from the origin with a small extent; all on one axis; all in one point
    P, T = c["cube_minus_face"]
    c["far_cube"] = (1.0e6 + 1.0e-3 * P, T)
    P, T = sheet(5, 4, holes=((2, 1), (2, 2)))
    c["flat_sheet"] = (P, T)
    c["on_one_axis"] = (np.stack([np.arange(len(P)) * 0.37 - 3.0, np.zeros(len(P)), np.zeros(len(P))], 1), T)
    c["in_one_point"] = (np.full((len(P), 3), 0.25), T)
    c["tiny_extent"] = (1.0e-300 * P, T)
    return c


# cases that also run with limits: name -> (hole_size, max_hole_edges) pairs; "extent:<k>" is resolved by limits()
LIMITED = {"cylinder": ((None, 13), (None, 14), (None, 7), (None, 6), (None, 0), ("extent:0", None),
                        ("below:0", None), ("extent:1", None), ("below:1", None), (0.0, None), (np.inf, None)),
           "cylinder_shuffled_1": ((None, 13), ("below:1", None)),
           "cylinder_shuffled_2": ((None, 13), ("extent:0", None)),
           "figure_eight": ((None, 4), (None, 3), (1.5, None)),
           "cones_65_129": ((None, 65), (None, 128), (None, 129)),
           "single_triangle": ((None, 3), (None, 2)),
           "in_one_point": ((0.0, None),),
           "far_cube": ((1.0e-3, None), (2.0e-3, None))}


def limits(name, spec):
    """-> (hole_size, max_hole_edges) of a LIMITED entry: "extent:k" is exactly the extent of the case's k-th
    component (the limit is inclusive), "below:k" the next double below it."""
    from tests import meshfill_oracle as fo
    size, edges = spec
    if isinstance(size, str):
        kind, k = size.split(":")
        P, T = cases()[name]
        e = float(fo.boundary_loops(P, T)["extent"][int(k)])
        size = e if kind == "extent" else float(np.nextafter(e, -np.inf))
    return size, edges


def runs():
    """Every (name, hole_size spec, max_hole_edges) the suites run."""
    out = [(name, None, None) for name in cases()]
    for name, specs in LIMITED.items():
        out += [(name, *spec) for spec in specs]
    return out


def run_id(run):
    name, size, edges = run
    return name + ("" if size is None else f"-size_{size}") + ("" if edges is None else f"-edges_{edges}")


@functools.lru_cache(maxsize=None)
def reference(run):
    """The oracle's (vertices, triangles, counts) of a run, computed once per process."""
    from tests import meshfill_oracle as fo
    name, size, edges = run
    P, T = cases()[name]
    size, edges = limits(name, (size, edges))
    return fo.fill_holes(P, T, hole_size=size, max_hole_edges=edges)


@functools.lru_cache(maxsize=None)
def reference_loops(name):
    from tests import meshfill_oracle as fo
    P, T = cases()[name]
    return fo.boundary_loops(P, T)


BAD_LIMITS = ((-1.0, None), (float("nan"), None), (-np.inf, None), (None, -1))
