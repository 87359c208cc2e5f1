"""CPU restatement of the Poisson meshing of csrc/slmesh.inl, in NumPy.

Kazhdan's FFT Poisson reconstruction on a dense periodic R^3 grid, R =
2^depth, with marching tetrahedra over the six Kuhn tetrahedra of every cube.
Open3D's create_from_point_cloud_poisson is the adaptive-octree variant and is
not installed here, so parity with Open3D is UNPINNED: this file is the
reference the GPU is checked against -- bit for bit for every stage except the
FFT solve, which is checked to a tolerance.  Every operation is the IEEE
operation slmesh.inl's header names, in its order; NumPy's elementwise ``+ - *
/``, ``floor`` and ``rint`` are exactly those.
"""
from __future__ import annotations

import struct

import numpy as np

from tests.plane_oracle import ordered_sum

FIX = 2.0 ** 30          # the splat's fixed-point scale
FIX_MAX = 2.0 ** 62      # a contribution at or beyond it (or NaN) adds 0
# the Kuhn tetrahedra: the axis permutations in lexicographic order; the
# tetrahedron of (a1, a2, a3) has the cube corners 0, bit a1, bit a1 | bit a2, 7
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
EVEN = (True, False, False, True, True, False)   # det(e_a1, e_a2, e_a3) > 0
TET_CORNERS = tuple((0, 1 << p[0], (1 << p[0]) | (1 << p[1]), 7) for p in PERMS)


def _even(seq) -> bool:
    inv = sum(1 for i in range(len(seq)) for j in range(i + 1, len(seq)) if seq[i] > seq[j])
    return inv % 2 == 0


def case_table():
    """Row m (bit q set: local corner q inside) -> the triangles of a
    positively oriented tetrahedron, each three edges (p, q), p < q, wound so
    that the normal points to the outside corners."""
    rows = []
    for m in range(16):
        ins = [q for q in range(4) if (m >> q) & 1]
        outs = [q for q in range(4) if not (m >> q) & 1]
        e = lambda a, b: (min(a, b), max(a, b))  # noqa: E731
        if len(ins) == 1:
            q, r = ins[0], list(outs)
            if not _even([q] + r):
                r[1], r[2] = r[2], r[1]
            rows.append([(e(q, r[0]), e(q, r[1]), e(q, r[2]))])
        elif len(ins) == 3:
            q, r = outs[0], list(ins)
            if not _even([q] + r):
                r[1], r[2] = r[2], r[1]
            rows.append([(e(q, r[0]), e(q, r[2]), e(q, r[1]))])
        elif len(ins) == 2:
            a, b = ins
            c, d = outs
            if not _even([a, b, c, d]):
                c, d = d, c
            rows.append([(e(a, c), e(a, d), e(b, d)), (e(a, c), e(b, d), e(b, c))])
        else:
            rows.append([])
    return rows


CASES = case_table()
EDGE_INDEX = {(0, 1): 0, (0, 2): 1, (0, 3): 2, (1, 2): 3, (1, 3): 4, (2, 3): 5}


def box(points, depth: int, scale: float = 1.1):
    """-> (origin f64 [3], h, R)."""
    P = np.asarray(points, dtype=np.float64)
    R = 1 << depth
    lo, hi = P.min(0), P.max(0)
    c = (lo + hi) / 2.0
    L = scale * float((hi - lo).max())
    if not L > 0.0:
        L = 1.0
    h = L / R
    return c - L / 2.0, h, R


CELL_MAX = 9.0e18       # a floor at or beyond it (or NaN) is cell 0: every other one is an int64


def _cell(P, origin, h):
    """corners() of slmesh.inl: fl = floor(g); the cell is int64(fl) where |fl|
    < 9.0e18, else 0 (NaN too); f = g - fl (NaN for a NaN or infinite g).  The
    cell is wrapped by the caller's ``& (R - 1)``."""
    with np.errstate(invalid="ignore", over="ignore"):
        g = (np.asarray(P, dtype=np.float64) - origin) / h
        fl = np.floor(g)
        f = g - fl
        ok = np.abs(fl) < CELL_MAX
    return np.where(ok, fl, 0.0).astype(np.int64), f


def _corner_weight(f, c):
    wx = f[:, 0] if c & 1 else 1.0 - f[:, 0]
    wy = f[:, 1] if c & 2 else 1.0 - f[:, 1]
    wz = f[:, 2] if c & 4 else 1.0 - f[:, 2]
    return (wx * wy) * wz


def _corner_index(i0, c, R):
    i = (i0[:, 0] + (c & 1)) & (R - 1)
    j = (i0[:, 1] + ((c >> 1) & 1)) & (R - 1)
    k = (i0[:, 2] + ((c >> 2) & 1)) & (R - 1)
    return (i * R + j) * R + k


def _fix(v):
    """fix() of slmesh.inl: |t| < 2^62 ? rint(t) : 0 with t = v 2^30 (so an
    infinite or NaN t adds 0); no operation here warns on such a t."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(v, dtype=np.float64) * FIX
        ok = np.abs(t) < FIX_MAX
    return np.rint(np.where(ok, t, 0.0)).astype(np.int64)


def splat(points, normals, origin, h, R):
    """-> (W f32 [R,R,R], V f32 [3,R,R,R]): 64-bit fixed-point sums."""
    G = unfix(splat_sums(points, normals, origin, h, R)).reshape(4, R, R, R)
    return G[0], G[1:]


def splat_sums(points, normals, origin, h, R):
    """The splat's accumulators -> int64 [4, R^3] (W, V_x, V_y, V_z); the sums wrap."""
    N = np.asarray(normals, dtype=np.float64)
    i0, f = _cell(points, origin, h)
    acc = np.zeros((4, R * R * R), dtype=np.int64)
    for c in range(8):
        w = _corner_weight(f, c)
        lin = _corner_index(i0, c, R)
        np.add.at(acc[0], lin, _fix(w))
        for a in range(3):
            with np.errstate(invalid="ignore", over="ignore"):  # 0 inf, and a NaN weight: fix gives 0
                wn = w * N[:, a]
            np.add.at(acc[1 + a], lin, _fix(wn))
    return acc


def unfix(acc):
    """float(double(sum) 2^-30) of every accumulator."""
    return (np.asarray(acc, dtype=np.int64).astype(np.float64) * (1.0 / FIX)).astype(np.float32)


def divergence(V, h):
    V = np.asarray(V, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):  # inf - inf is NaN, as on the device
        dx = np.roll(V[0], -1, 0) - np.roll(V[0], 1, 0)
        dy = np.roll(V[1], -1, 1) - np.roll(V[1], 1, 1)
        dz = np.roll(V[2], -1, 2) - np.roll(V[2], 1, 2)
        s = (dx + dy) + dz
        assert s.dtype == np.float32
        return (s.astype(np.float64) / (2.0 * h)).astype(np.float32)


def eigenvalues(R, h, dtype=np.float64):
    c = (2.0 * np.cos(2.0 * np.pi * np.arange(R) / R) - 2.0).astype(dtype)
    lam = (c[:, None, None] + c[None, :, None]) + c[None, None, : R // 2 + 1]
    return lam / dtype(h * h)


def solve(div, h):
    """The f64 solve of an f32 divergence -> chi f64 [R,R,R]."""
    d = np.asarray(div, dtype=np.float64)
    R = d.shape[0]
    lam = eigenvalues(R, h)
    lam[0, 0, 0] = 1.0
    F = np.fft.rfftn(d) / lam
    F[0, 0, 0] = 0.0
    return np.fft.irfftn(F, s=d.shape, axes=(0, 1, 2))


def sample(grid, points, origin, h):
    """Trilinear grid value at every point, f64, the eight corners added to 0.0 in corner order."""
    G = np.asarray(grid)
    R = G.shape[0]
    flat = G.reshape(-1).astype(np.float64)
    i0, f = _cell(points, origin, h)
    acc = np.zeros(len(i0))
    with np.errstate(invalid="ignore"):  # 0 inf and inf - inf are NaN, as on the device
        for c in range(8):
            acc = acc + _corner_weight(f, c) * flat[_corner_index(i0, c, R)]
    return acc


def iso_value(chi, points, origin, h) -> float:
    return ordered_sum(sample(chi, points, origin, h)) / float(len(points))


def get_center(points):
    P = np.asarray(points, dtype=np.float64)
    return np.array([ordered_sum(P[:, a]) / float(len(P)) for a in range(3)])


def orient_towards(points, normals, location):
    P = np.asarray(points, dtype=np.float64)
    N = np.array(normals, dtype=np.float64)
    d = np.asarray(location, dtype=np.float64) - P
    dot = (N[:, 0] * d[:, 0] + N[:, 1] * d[:, 1]) + N[:, 2] * d[:, 2]
    zero = (N[:, 0] == 0.0) & (N[:, 1] == 0.0) & (N[:, 2] == 0.0)
    ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = np.where((ln == 0.0)[:, None], np.array([0.0, 0.0, 1.0]), d / ln[:, None])
    flip = ~zero & (dot < 0.0)
    N[flip] = -N[flip]
    N[zero] = unit[zero]
    return N


def _offsets(c):
    return c & 1, (c >> 1) & 1, (c >> 2) & 1


def _shift(a, c):
    """a at node + offsets(c), periodic."""
    di, dj, dk = _offsets(c)
    return np.roll(a, (-di, -dj, -dk), (0, 1, 2))


def extract(chi, iso, origin, h):
    """-> (vertices f64 [V,3], triangles int32 [T,3])."""
    chi = np.asarray(chi, dtype=np.float32)
    R = chi.shape[0]
    origin = np.asarray(origin, dtype=np.float64)
    with np.errstate(invalid="ignore"):  # inf - inf (an infinite iso) is NaN: outside
        v = chi.astype(np.float64) - float(iso)
        inside = v < 0.0
    n3 = R * R * R
    crossed = np.zeros((n3, 7), dtype=bool)
    for d in range(1, 8):
        crossed[:, d - 1] = (inside != _shift(inside, d)).reshape(-1)
    cnt = crossed.sum(1)
    vpos = np.cumsum(cnt) - cnt
    vid = vpos[:, None] + (np.cumsum(crossed, 1) - crossed)
    node, dm1 = np.nonzero(crossed)
    i, j, k = node // (R * R), (node // R) % R, node % R
    idx = np.stack([i, j, k], 1).astype(np.float64)
    off = np.stack([(dm1 + 1) & 1, ((dm1 + 1) >> 1) & 1, ((dm1 + 1) >> 2) & 1], 1).astype(np.float64)
    pa = origin + h * idx
    pb = origin + h * (idx + off)
    va = v.reshape(-1)[node]
    nb = ((((i + ((dm1 + 1) & 1)) & (R - 1)) * R + ((j + (((dm1 + 1) >> 1) & 1)) & (R - 1))) * R
          + ((k + (((dm1 + 1) >> 2) & 1)) & (R - 1)))
    vb = v.reshape(-1)[nb]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):  # a NaN or infinite node: NaN vertices
        t = va / (va - vb)
        verts = pa + (pb - pa) * t[:, None]

    corner_in = [_shift(inside, c).reshape(-1) for c in range(8)]
    lin = np.arange(n3).reshape(R, R, R)
    corner_node = [_shift(lin, c).reshape(-1) for c in range(8)]
    tri_ok = np.zeros((n3, 6, 2), dtype=bool)
    tri = np.zeros((n3, 6, 2, 3), dtype=np.int64)
    for t_i, corners in enumerate(TET_CORNERS):
        m = sum(corner_in[corners[q]].astype(np.int64) << q for q in range(4))
        for case in range(1, 15):
            sel = np.nonzero(m == case)[0]
            if not len(sel):
                continue
            for k_i, edges in enumerate(CASES[case]):
                if not EVEN[t_i]:
                    edges = (edges[0], edges[2], edges[1])
                tri_ok[sel, t_i, k_i] = True
                for s, (p, q) in enumerate(edges):
                    ca, cb = corners[p], corners[q]
                    tri[sel, t_i, k_i, s] = vid[corner_node[ca][sel], (ca ^ cb) - 1]
    return verts, tri[tri_ok].astype(np.int32)


def tet_cases(chi, iso):
    """The set of tetrahedron cases (0..15) a field produces."""
    inside = (np.asarray(chi, dtype=np.float32).astype(np.float64) - float(iso)) < 0.0
    corner_in = [_shift(inside, c).reshape(-1) for c in range(8)]
    seen = set()
    for corners in TET_CORNERS:
        seen |= set(np.unique(sum(corner_in[corners[q]].astype(np.int64) << q for q in range(4))).tolist())
    return seen


def tet_pairs(chi, iso):
    """The set of (tetrahedron q, case m), q = 0..5, m = 1..14, a field produces
    (84 at the most: the winding swap of t1, t2, t5 is per tetrahedron)."""
    with np.errstate(invalid="ignore"):
        inside = (np.asarray(chi, dtype=np.float32).astype(np.float64) - float(iso)) < 0.0
    corner_in = [_shift(inside, c).reshape(-1) for c in range(8)]
    seen = set()
    for q, corners in enumerate(TET_CORNERS):
        m = np.unique(sum(corner_in[corners[r]].astype(np.int64) << r for r in range(4)))
        seen |= {(q, int(x)) for x in m if 0 < x < 15}
    return seen


def lerp_quantile(sorted_lo: float, sorted_hi: float, gamma: float) -> float:
    """numpy.quantile's linear interpolation between the two sorted neighbours."""
    a, b, t = float(sorted_lo), float(sorted_hi), float(gamma)
    d = b - a
    return b - d * (1.0 - t) if t >= 0.5 else a + d * t


def quantile(values, q: float) -> float:
    s = np.sort(np.asarray(values, dtype=np.float64))
    pos = q * (len(s) - 1)
    lo = int(np.floor(pos))
    hi = min(lo + 1, len(s) - 1)
    return lerp_quantile(s[lo], s[hi], pos - lo)


def remove_vertices_by_mask(vertices, triangles, mask):
    """A triangle with an index outside 0 .. len(vertices) - 1 is dropped; such
    an index is never used to index anything."""
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    keep = ~mask
    new = np.cumsum(keep) - keep
    T = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    inside = (T >= 0) & (T < len(keep))
    tk = np.zeros(len(T), dtype=bool)
    if len(keep):
        tk = (inside & keep[np.where(inside, T, 0)]).all(1)
    return np.asarray(vertices).reshape(-1, 3)[keep], new[T[tk]].astype(np.int32).reshape(-1, 3)


def poisson(points, normals, depth, scale=1.1, chi=None):
    """The whole chain -> dict; ``chi`` replaces the f64 solve (an f32 field of another solver)."""
    origin, h, R = box(points, depth, scale)
    W, V = splat(points, normals, origin, h, R)
    div = divergence(V, h)
    if chi is None:
        chi = solve(div, h).astype(np.float32)
    iso = iso_value(chi, points, origin, h)
    verts, tris = extract(chi, iso, origin, h)
    dens = sample(W, verts, origin, h)
    return {"origin": origin, "h": h, "R": R, "W": W, "V": V, "div": div, "chi": chi, "iso": iso,
            "vertices": verts, "triangles": tris, "densities": dens}


def triangle_normals(vertices, triangles):
    """Unit f64 normals of the f64 vertices, zero for a zero-area triangle."""
    P = np.asarray(vertices, dtype=np.float64)
    T = np.asarray(triangles)
    e1, e2 = P[T[:, 1]] - P[T[:, 0]], P[T[:, 2]] - P[T[:, 0]]
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where((ln == 0.0)[:, None], 0.0, n / ln[:, None])


def stl_bytes(vertices, triangles) -> bytes:
    """Binary STL, one record at a time (the slow, obvious way)."""
    P = np.asarray(vertices, dtype=np.float64)
    T = np.asarray(triangles)
    N = triangle_normals(P, T) if len(T) else np.zeros((0, 3))
    out = [b"\0" * 80, struct.pack("<I", len(T))]
    for t in range(len(T)):
        rec = [np.float32(x) for x in N[t]] + [np.float32(x) for vtx in T[t] for x in P[vtx]]
        out.append(struct.pack("<12fH", *rec, 0))
    return b"".join(out)


# ---- properties of a mesh -------------------------------------------------------------------------------------
def edge_census(triangles):
    """-> (closed, E): closed iff every undirected edge is in exactly two triangles, once in each direction."""
    T = np.asarray(triangles, dtype=np.int64)
    a = np.concatenate([T[:, 0], T[:, 1], T[:, 2]])
    b = np.concatenate([T[:, 1], T[:, 2], T[:, 0]])
    big = int(T.max()) + 1 if len(T) else 1
    directed = a * big + b
    if len(np.unique(directed)) != len(directed):
        return False, 0
    und, counts = np.unique(np.minimum(a, b) * big + np.maximum(a, b), return_counts=True)
    rev = np.isin(b * big + a, directed)
    return bool((counts == 2).all() and rev.all()), len(und)


def signed_volume(vertices, triangles) -> float:
    P = np.asarray(vertices, dtype=np.float64)
    T = np.asarray(triangles)
    return float(np.einsum("ij,ij->i", P[T[:, 0]], np.cross(P[T[:, 1]], P[T[:, 2]])).sum() / 6.0)


def sphere(n=20000, centre=(0.1, -0.2, 0.3), seed=0):
    """n points of the unit sphere about ``centre`` with outward normals."""
    rng = np.random.default_rng(seed)
    N = rng.normal(size=(n, 3))
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    return N + np.asarray(centre), N
