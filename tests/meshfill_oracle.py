"""CPU restatement of the hole filling of csrc/slmeshfill.inl, in NumPy: the definition.

Open3D's tensor fill_holes(hole_size) is not installed here, so parity with it is UNPINNED; this file is what the GPU
is checked against, exactly.  Nothing below depends on the order in which sides, loops or vertices are visited.

boundary side  a side a->b of a triangle whose edge key has one side in all (meshcheck_oracle's m = 1; a degenerate
               triangle (a, a, b) gives the self-loop a->a).
simple vertex  exactly one boundary side leaves it and exactly one enters it.
component      boundary sides that share an end vertex, in either role, are joined.  Its LABEL is its smallest vertex,
               its SIZE n its number of sides, its EXTENT the diagonal sqrt((dx dx + dy dy) + dz dz) of the box of
               its vertices.  It is a SIMPLE LOOP iff every vertex it touches is simple.
eligible       a simple loop with 3 <= n <= 2^22, n <= max_hole_edges and extent <= hole_size (where given).
cap            n = 3, a -> b -> c -> a with a the label: the triangle (a, c, b).  n > 3: one new vertex at the
               centroid and per side a -> b the triangle (b, a, centre).
centroid       lo = the minimum over ALL vertices of the mesh, e = the largest component of max - lo, s = 2^(40 - k)
               with e < 2^k (frexp; e = 0: s = 1; k is taken as at least -983 so that s is finite).  Per component
               S = the int64 sum of rint((x - lo) s) over the loop's vertices; the centre is lo + (S / n) / s.
order          old vertices, then the new ones in ascending label; old triangles, then the new ones in ascending
               from-vertex (the one triangle of an n = 3 loop at its label).
"""
from __future__ import annotations

import math

import numpy as np

from tests import meshcheck_oracle as ko

MAX_LOOP_SIDES = 1 << 22
COUNT_KEYS = ("components", "simple_loops", "filled", "skipped_not_simple", "skipped_by_limit", "new_vertices",
              "new_triangles", "boundary_sides")


def boundary_sides(triangles, n_vertices):
    """-> (from, to) int64 [B]: the sides whose key occurs once, in ascending key order."""
    T = ko.check_indices(triangles, n_vertices)
    keys, _, _, cf, ct = ko._sorted_sides(T, n_vertices)
    start, m = ko._runs(keys)
    one = start[m == 1]
    flat = T.reshape(-1).astype(np.int64)
    return flat[cf[one]], flat[ct[one]]


def _vertices(vertices, n_vertices):
    P = None if vertices is None else np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    V = len(P) if n_vertices is None else int(n_vertices)
    if P is not None and not np.isfinite(P).all():
        raise ValueError("non-finite vertex coordinates")
    return P, V


def _components(frm, to, V):
    """-> per side its component's label (the smallest vertex of the component)."""
    parent = np.arange(V)
    for a, b in zip(frm.tolist(), to.tolist()):
        a, b = ko._find(parent, a), ko._find(parent, b)
        if a != b:
            parent[max(a, b)] = min(a, b)          # the smaller index is the root: a root is its class' minimum
    return np.array([ko._find(parent, a) for a in frm.tolist()], dtype=np.int64)


def _loops(P, frm, to, V):
    """-> (label [C] ascending, size [C], simple [C], extent [C] | None, the component row of every side)."""
    lab = _components(frm, to, V)
    label, row, size = np.unique(lab, return_inverse=True, return_counts=True)
    out_deg, in_deg = np.bincount(frm, minlength=V), np.bincount(to, minlength=V)
    plain = (out_deg == 1) & (in_deg == 1)
    bad = np.zeros(len(label), dtype=bool)
    np.logical_or.at(bad, row, ~(plain[frm] & plain[to]))
    extent = None
    if P is not None:
        lo, hi = np.full((len(label), 3), np.inf), np.full((len(label), 3), -np.inf)
        for ends in (frm, to):
            np.minimum.at(lo, row, P[ends])
            np.maximum.at(hi, row, P[ends])
        d = hi - lo
        extent = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return label, size, ~bad, extent, row


def boundary_loops(vertices, triangles, n_vertices=None) -> dict:
    """One row per boundary component in ascending label: label int32, size int64, simple bool, and extent f64 when
    vertices are given."""
    P, V = _vertices(vertices, n_vertices)
    frm, to = boundary_sides(triangles, V)
    label, size, simple, extent, _ = _loops(P, frm, to, V)
    out = {"label": label.astype(np.int32), "size": size.astype(np.int64), "simple": simple.astype(bool)}
    if extent is not None:
        out["extent"] = extent.astype(np.float64)
    return out


def check_limits(hole_size, max_hole_edges):
    if hole_size is not None and not float(hole_size) >= 0.0:
        raise ValueError("hole_size must be a number >= 0")
    if max_hole_edges is not None and int(max_hole_edges) < 0:
        raise ValueError("max_hole_edges must be >= 0")


def fixed_point_scale(P):
    """-> (lo f64 [3], s): the origin and the power of two of the centroid sums."""
    lo, hi = P.min(0), P.max(0)
    with np.errstate(over="ignore"):
        e = float((hi - lo).max())
    if not math.isfinite(e):
        raise ValueError("the extent of the vertices is not finite")
    if e == 0.0:
        return lo, 1.0
    k = max(math.frexp(e)[1], -983)
    return lo, math.ldexp(1.0, 40 - k)


def fill_holes(vertices, triangles, hole_size=None, max_hole_edges=None):
    """-> (vertices f64 [V', 3], triangles int32 [T', 3], counts)."""
    check_limits(hole_size, max_hole_edges)
    P, V = _vertices(vertices, None)
    T = ko.check_indices(triangles, V).astype(np.int32).reshape(-1, 3)
    counts = dict.fromkeys(COUNT_KEYS, 0)
    frm, to = boundary_sides(T, V)
    counts["boundary_sides"] = len(frm)
    if len(frm) == 0:
        return P.copy(), T.copy(), counts
    lo, s = fixed_point_scale(P)
    label, size, simple, extent, row = _loops(P, frm, to, V)
    ok = simple & (size >= 3) & (size <= MAX_LOOP_SIDES)
    if max_hole_edges is not None:
        ok &= size <= int(max_hole_edges)
    if hole_size is not None:
        ok &= extent <= float(hole_size)
    fan = ok & (size > 3)
    S = np.zeros((len(label), 3), dtype=np.int64)
    np.add.at(S, row, np.rint((P[frm] - lo) * s).astype(np.int64))          # a simple loop: every vertex leaves once
    centre = lo + (S.astype(np.float64) / size.astype(np.float64)[:, None]) / s
    new_index = V + np.cumsum(fan) - fan                                     # ascending label
    # the fans, one triangle per side, and the single triangles: both keyed by the from-vertex they are placed at
    in_fan = fan[row]
    place = [frm[in_fan]]
    tris = [np.stack([to[in_fan], frm[in_fan], new_index[row[in_fan]]], 1)]
    three = np.nonzero(ok & (size == 3))[0]
    if len(three):
        first = np.isin(row, three) & (frm == label[row])                    # the side a -> b that leaves the label
        a, b = frm[first], to[first]
        nxt = np.full(V, -1, dtype=np.int64)
        nxt[frm] = to                                                        # (read at simple vertices only)
        place.append(a)
        tris.append(np.stack([a, nxt[b], b], 1))
    place, tris = np.concatenate(place), np.concatenate(tris)
    tris = tris[np.argsort(place, kind="stable")]
    counts.update(components=len(label), simple_loops=int(simple.sum()), filled=int(ok.sum()),
                  skipped_not_simple=int((~simple).sum()), skipped_by_limit=int((simple & ~ok).sum()),
                  new_vertices=int(fan.sum()), new_triangles=len(tris))
    return (np.concatenate([P, centre[fan]]).astype(np.float64).reshape(-1, 3),
            np.concatenate([T, tris.astype(np.int32)]).astype(np.int32).reshape(-1, 3), counts)
