"""Inputs that drive the Poisson meshing kernels (csrc/slmesh.inl) down the
paths a cloud inside its own bounding box never takes, shared by
tests/test_mesh_oracle.py (which proves on the CPU, from tests/mesh_oracle.py
alone, that each input meets its precondition) and
tests/test_gpu_mesh_paths.py (which compares the library with the oracle on
the same inputs, bit for bit).

The direct-call cases use the origin (0, 0, 0) and h = 1 (or another power of
two), so that g = (p - o) / h is exact, and put each special contribution on a
node of its own, so that the sums stay isolated.  Everything returned is
deterministic; cached arrays are read only.
"""
from __future__ import annotations

import functools
import math

import numpy as np

from tests import mesh_oracle as mo

ZERO3 = np.zeros(3)
SEAM_ORIGIN, SEAM_H = np.array([0.3, -1.7, 2.9]), 0.37   # test_gpu_mesh.py's extraction box


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ------------------------------------------------------------------ clouds ----
def cloud(kind, n, R, seed):
    """-> (points, normals, scale): the clouds of test_splat_and_divergence_bits."""
    rng = np.random.default_rng(seed)
    N = rng.normal(size=(n, 3))
    scale = 1.1
    if kind == "nodes":  # scale 1 and extents R: h = 1, origin 0, every point on a node
        P = rng.integers(0, R + 1, size=(n, 3)).astype(np.float64)
        P[0] = 0.0
        P[-1] = R  # (n = 1: a single point, the unit box about it)
        scale = 1.0
    elif kind == "faces":  # scale 1: the points of the bounding box's faces lie on the grid's seam
        P = rng.random((n, 3)) * 3.0 - 1.0
        P[rng.random((n, 3)) < 0.25] = 2.0
        P[rng.random((n, 3)) < 0.25] = -1.0
        scale = 1.0
    elif kind == "onecell":  # two corner points fix the box; the rest share one cell
        P = 0.4 + 1e-3 * rng.random((n, 3))
        P[0] = 0.0
        P[-1] = 1.0
    else:  # "flat": a zero-extent axis
        P = rng.random((n, 3))
        P[:, 1] = 0.25
    return P, N, scale


CLOUD_KINDS = ("nodes", "faces", "onecell", "flat")


# ------------------------------------------------------------- splat cases ----
# the coordinates of "outside" (the last two finite ones are there because their
# cells are not 0 at a large magnitude)
OUTSIDE = (-0.25, -1.5, -5.0, "R", "R+0.5", 9.75, 1e19, -1e19, 9.1e18, 8.9e18, -8.9e18, 2.0 ** 62, -3e9, 5e12,
           5e12 + 3.5, -3e9 - 0.5, float("nan"), float("inf"), float("-inf"))
SAT_EDGE = float(np.nextafter(2.0 ** 32, 0.0))   # 2^32 - 2^-21: times 2^30 it is 2^62 - 2^9, added
SATURATE = (SAT_EDGE, 2.0 ** 32, -2.0 ** 32, float("inf"), float("-inf"), float("nan"))  # all but the first add 0


def outside_coordinates(R):
    return np.array([float(R) if c == "R" else R + 0.5 if c == "R+0.5" else c for c in OUTSIDE])


def expected_cell(x, R):
    """corners()'s rule in Python's exact integers: the wrapped cell of the coordinate x (origin 0, h 1)."""
    if not math.isfinite(x) or abs(math.floor(x)) >= 9 * 10 ** 18:
        return 0
    return math.floor(x) % R


def outside_points(R):
    """Every coordinate on every axis beside two plain ones, then all three at once (cyclic triples)."""
    c = outside_coordinates(R)
    rows = []
    for a in range(3):
        for x in c:
            p = [0.25, 1.5, 0.75]
            p[a] = x
            rows.append(p)
    for t in range(len(c)):
        rows.append([c[t], c[(t + 5) % len(c)], c[(t + 11) % len(c)]])
    return np.array(rows)


@functools.lru_cache(maxsize=None)
def splat_case(name):
    """-> (points, normals, depth); origin (0, 0, 0), h = 1."""
    if name == "ties":  # every w 2^30 and w n_x 2^30 is an odd half
        k = np.arange(20.0)
        P = np.stack([1.0 + (2.0 * k + 1.0) * 2.0 ** -31, np.full(20, 2.0), np.full(20, 1.0)], 1)
        N = np.tile([1.0, -1.0, 0.5], (20, 1))
        return _ro(P, N) + (2,)
    if name == "saturate":  # 18 nodes: each value in each component, 0.25 in the two others
        P, N = [], []
        for t, v in enumerate(SATURATE):
            for a in range(3):
                P.append([t % 4, a, t // 4])
                n = [0.25, 0.25, 0.25]
                n[a] = v
                N.append(n)
        return _ro(np.array(P, dtype=np.float64), np.array(N)) + (2,)
    if name == "wrap":  # 4 x 2^61 = 2^63 wraps to -2^63; 4 x -2^61 = -2^63 does not wrap
        P = np.tile([3.0, 1.0, 2.0], (4, 1))
        N = np.tile([2.0 ** 31, -2.0 ** 31, 0.5], (4, 1))
        return _ro(P, N) + (2,)
    if name.startswith("outside"):  # "outside1", "outside3": depth 1 and 3
        depth = int(name[len("outside"):])
        P = outside_points(1 << depth)
        N = np.random.default_rng(40 + depth).normal(size=P.shape)
        return _ro(P, N) + (depth,)
    raise KeyError(name)


SPLAT_CASES = ("ties", "saturate", "wrap", "outside1", "outside3")


# ------------------------------------------------------------------ fields ----
@functools.lru_cache(maxsize=None)
def fields():
    """name -> (chi f32 [R, R, R], iso).  "random", "on_iso", "seam", "constant"
    are test_extraction_bits' fields (R = 8, default_rng(11))."""
    rng = np.random.default_rng(11)
    R = 8
    i, j, k = np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij")
    wrapped = lambda a: np.minimum(a, R - a)  # noqa: E731  (periodic distance to node 0)
    out = {
        "random": (rng.normal(size=(R, R, R)).astype(np.float32), 0.0),
        "on_iso": (rng.integers(-1, 2, size=(R, R, R)).astype(np.float32) + 0.5, 0.5),
        "seam": (np.sqrt(wrapped(i) ** 2 + wrapped(j) ** 2 + wrapped(k) ** 2).astype(np.float32), 2.3),
        "constant": (np.full((R, R, R), 0.25, np.float32), 0.25),
        # default_rng(1) at R = 4 gives all 84 (tetrahedron, case) pairs
        "random4": (np.random.default_rng(1).normal(size=(4, 4, 4)).astype(np.float32), 0.0),
        "on_iso4": (np.random.default_rng(2).integers(-1, 2, size=(4, 4, 4)).astype(np.float32) + 0.5, 0.5),
    }
    for s in range(4):  # R = 2: every cube's corners wrap onto the opposite nodes
        out[f"random2_{s}"] = (np.random.default_rng(20 + s).normal(size=(2, 2, 2)).astype(np.float32), 0.0)
    out["on_iso2"] = (np.random.default_rng(3).integers(-1, 2, size=(2, 2, 2)).astype(np.float32) + 0.5, 0.5)
    out.update(_special_fields())
    for chi, _ in out.values():
        chi.setflags(write=False)
    return out


ALL_PAIRS = ("random", "random4")                      # all 84 (tetrahedron, case) pairs
CLOSED = ("random", "on_iso", "seam", "random4", "on_iso4", "random2_0", "random2_1", "random2_2", "random2_3",
          "on_iso2")                                   # every directed edge once, every undirected edge twice
SPECIAL = ("special_nonfinite", "special_zeros", "special_subnormal")
SUB = np.float32(1.4e-45)                              # the least f32 subnormal
# (node, value) of special_nonfinite; inside iff double(chi) - iso < 0: only -inf is
SPECIAL_NODES = (((0, 0, 0), np.nan), ((1, 2, 3), np.inf), ((2, 0, 1), -np.inf), ((3, 3, 3), np.nan),
                 ((0, 2, 2), np.inf), ((3, 1, 0), -np.inf))
ZERO_NODES = (((0, 0, 0), -0.0), ((1, 1, 1), 0.0), ((2, 3, 1), -0.0), ((3, 0, 2), 0.0))


def _special_fields():
    base = np.random.default_rng(5).normal(size=(4, 4, 4)).astype(np.float32)
    nonfinite = base.copy()
    for node, v in SPECIAL_NODES:
        nonfinite[node] = v
    zeros = base.copy()
    for node, v in ZERO_NODES:
        zeros[node] = v
    # multiples -3 .. 3 of the least subnormal, and +-1e-38 (below the least normal, 1.18e-38): a build that
    # flushes f32 denormals sees zeros, which are outside
    rng = np.random.default_rng(6)
    sub = rng.integers(-3, 4, size=(4, 4, 4)).astype(np.float32) * SUB
    big = rng.random((4, 4, 4)) < 0.25
    sub[big] = np.where(rng.random(int(big.sum())) < 0.5, np.float32(1e-38), np.float32(-1e-38))
    return {"special_nonfinite": (nonfinite, 0.0), "special_zeros": (zeros, 0.0), "special_subnormal": (sub, 0.0)}


@functools.lru_cache(maxsize=None)
def divergence_fields():
    """name -> (V f32 [3, 4, 4, 4], h): differences that are subnormal, and non-finite nodes."""
    rng = np.random.default_rng(7)
    V = np.zeros((3, 4, 4, 4), np.float32)
    V[0] = rng.integers(-5, 6, size=(4, 4, 4)).astype(np.float32) * SUB
    V[1] = rng.integers(-1, 2, size=(4, 4, 4)).astype(np.float32) * np.float32(1e-38)
    V[2] = rng.integers(-5, 6, size=(4, 4, 4)).astype(np.float32) * np.float32(2e-45)
    V[0, 2, 1, 1], V[0, 0, 1, 1] = 3e-45, 1.4e-45   # two nodes apart: node (1, 1, 1)'s dx is one subnormal step
    V[1, 1, 2, 1], V[1, 1, 0, 1] = 1e-38, 0.0
    V[2, 1, 1, 2], V[2, 1, 1, 0] = 0.0, 0.0
    W = rng.normal(size=(3, 4, 4, 4)).astype(np.float32)
    W[0, 0, 0, 0], W[1, 1, 2, 3], W[2, 3, 3, 3], W[0, 2, 2, 2] = np.nan, np.inf, -np.inf, np.inf
    W[0, 0, 2, 2] = np.inf                          # inf - inf across node (1, 2, 2)
    return {"subnormal": (_ro(V), 1.0), "subnormal_h": (_ro(V.copy()), 0.37), "nonfinite": (_ro(W), 0.5)}


# ----------------------------------------------------------- sample points ----
PERIODIC_ORIGIN, PERIODIC_H = np.array([-1.0, 0.5, 2.0]), 0.5


@functools.lru_cache(maxsize=None)
def periodic_points(R=8, n=300):
    """p on a 2^-20 h lattice of the box (h = 0.5, so every shift by h R is
    exact) -> (p, [shifted copies]): p - h R e_a, p + h R e_a, p + 2 h R e_a."""
    rng = np.random.default_rng(8)
    p = PERIODIC_ORIGIN + rng.integers(0, R << 20, size=(n, 3)).astype(np.float64) * (PERIODIC_H * 2.0 ** -20)
    shifted = []
    for a in range(3):
        e = np.zeros(3)
        e[a] = PERIODIC_H * R
        shifted += [p - e, p + e, p + 2.0 * e]
    return _ro(p), shifted


@functools.lru_cache(maxsize=None)
def seam_vertices():
    """The "seam" field's own vertices (the oracle's), in test_extraction_bits' box."""
    chi, iso = fields()["seam"]
    return _ro(mo.extract(chi, iso, SEAM_ORIGIN, SEAM_H)[0])


# -------------------------------------------------------------- trim cases ----
TRIM_COUNTS = (0, 1, 4095, 4096, 4097)    # around the scan's tile (kRsTile = 4096)
TRIM_MASKS = ("none", "all", "alternating", "one")
INT32_MAX = 2 ** 31 - 1


def trim_case(nv, nt, mask):
    """-> (vertices f64 [nv, 3], triangles int32 [nt, 3], mask bool [nv]).
    Every fifth triangle has an index outside the mesh (-1, nv, 2^31 - 1 in
    turn, the slot in turn); every seventh repeats a vertex."""
    rng = np.random.default_rng(1000 * nv + nt)
    V = rng.normal(size=(nv, 3))
    T = rng.integers(0, max(nv, 1), size=(nt, 3)).astype(np.int32)
    bad = (-1, nv, INT32_MAX)
    for t in range(0, nt, 5):
        T[t, (t // 5) % 3] = bad[(t // 15) % 3]
    for t in range(3, nt, 7):
        T[t, 1] = T[t, 0]
    if nv == 0:  # no index is inside an empty mesh
        T[:] = np.array(bad, dtype=np.int32)[rng.integers(0, 3, size=(nt, 3))]
    m = np.zeros(nv, dtype=bool)
    if mask == "all":
        m[:] = True
    elif mask == "alternating":
        m[::2] = True
    elif mask == "one" and nv:
        m[nv // 2] = True
    return V, T, m


# ------------------------------------------------------------- ordered sum ----
OSUM_N = (1, 255, 256, 257, 4095, 4096, 4097, 8192, 8193, 4096 * 256, 4096 * 256 + 1)
OSUM_STRIDES = ((1, 0), (3, 0), (3, 2), (7, 3))
# default_rng(seed) per n.  Seeds other than 0 were found by search on the CPU:
# the first for which the ordered sum differs from both numpy.sum and the left
# fold at every (stride, offset) (tests/test_mesh_oracle.py asserts it again).
# n = 1 cannot differ: 0.0 + v is v in every order.
OSUM_SEED = {1: 0, 255: 4, 256: 9, 257: 2, 4095: 0, 4096: 1, 4097: 1, 8192: 2, 8193: 0, 4096 * 256: 0,
             4096 * 256 + 1: 1}


@functools.lru_cache(maxsize=2)
def osum_values(n, seed=None):
    """7 n normals scaled by 10^U(-8, 8); the case (n, stride, offset) sums
    values[: stride n][offset::stride]."""
    rng = np.random.default_rng(OSUM_SEED[n] if seed is None else seed)
    return _ro(rng.normal(size=7 * n) * 10.0 ** rng.uniform(-8.0, 8.0, size=7 * n))


def osum_case(n, stride, offset, seed=None):
    """-> (the flat array handed to sl_ordered_sum, the n values it sums)."""
    v = osum_values(n, seed)[: stride * n]
    return v, v[offset::stride]


# ------------------------------------------------------------------ orient ----
ORIENT_N = (255, 256, 257)   # around one workgroup
ORIENT_LOCATION = np.array([0.5, -0.25, 2.0])


def orient_case(n):
    """-> (points, normals, location, rows): rows names the special points."""
    rng = np.random.default_rng(n)
    loc = ORIENT_LOCATION
    P = rng.normal(size=(n, 3)) * 3.0
    N = rng.normal(size=(n, 3))
    N[::7] = 0.0
    rows = {"dot_plus_zero": 1, "dot_minus_zero": 2, "negative_zero_normal": 3, "at_location": 7,
            "last_plus_zero": n - 1, "flipped": 4, "kept": 5}
    # d = loc - p = (1, 2, 3): (3 + 0) + -3 = +0
    P[1], N[1] = loc - np.array([1.0, 2.0, 3.0]), [3.0, 0.0, -1.0]
    # d = (+0, -2, -3): (-1 (+0) + 0 (-2)) + 0 (-3) = (-0 + -0) + -0 = -0
    P[2], N[2] = loc - np.array([0.0, -2.0, -3.0]), [-1.0, 0.0, 0.0]
    P[3], N[3] = loc - np.array([1.0, 2.0, 3.0]), [-0.0, 0.0, -0.0]   # a zero normal: towards the location
    P[4], N[4] = loc - np.array([1.0, 2.0, 3.0]), [0.0, 0.0, -1.0]    # dot -3: flipped
    P[5], N[5] = loc - np.array([1.0, 2.0, 3.0]), [0.0, 0.0, 1.0]     # dot +3: kept
    P[7], N[7] = loc, [0.0, 0.0, 0.0]                                  # -> (0, 0, 1)
    P[n - 1], N[n - 1] = loc - np.array([2.0, -1.0, 4.0]), [1.0, 2.0, 0.0]   # (2 + -2) + 0 = +0, the last thread
    return P, N, loc, rows


# ------------------------------------------------------------------- solve ----
SOLVE_H = 0.37
SOLVE_CASES = tuple((depth, seed, shift) for depth in (1, 2, 3) for seed in (0, 1) for shift in (0.0, 3.0))


def solve_case(depth, seed, shift):
    """-> div f32 [R, R, R]; ``shift`` 3.0 gives it a non-zero mean (chi^(0) = 0 removes it)."""
    R = 1 << depth
    d = np.random.default_rng(100 * depth + seed).normal(size=(R, R, R)).astype(np.float32)
    return d + np.float32(shift)
