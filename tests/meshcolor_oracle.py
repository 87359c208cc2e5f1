"""The CPU restatement of csrc/slmeshcolor.inl that the vertex colours are checked
against: the cloud-to-mesh colour transfer as a brute force over the cloud with
the folds written out as scalar loops, and the coloured binary PLY one record at
a time (on tests/meshwrite_oracle.py's vertex normals, imported, not restated).

Open3D is not installed: its coloured PLY layout (uchar red green blue after nz)
is restated from memory and unpinned, and the transfer is this project's own
definition (Open3D's Poisson colours come from its octree's data field).
"""
from __future__ import annotations

import math
import struct

import numpy as np

from tests.meshwrite_oracle import vertex_normals

MAX_K = 16
FILL = (128, 128, 128)
UNRESOLVED = 255


def _d2(P, q):
    """((dx dx + dy dy) + dz dz) of q against every row of P, f64."""
    d = q[None, :] - P
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def tier_limit(P, Q, radius):
    """t_max: the smallest t with radius 2^t > diag of the joint bounding box of the cloud and the finite queries."""
    finite = np.isfinite(Q).all(1)
    J = np.concatenate([P, Q[finite]])
    e = J.max(0) - J.min(0)
    diag = math.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    t = 0
    while not math.ldexp(radius, t) > diag and t < 4096:
        t += 1
    return t


def candidates(P, q, radius, last_tier):
    """-> (tier, [(d2, index), ...] ascending, all of the tier's ball) or (255, []) when no tier up to last_tier
    (inclusive) has a point in its open ball."""
    d2 = _d2(P, q)
    for t in range(last_tier + 1):
        rt = math.ldexp(radius, t)
        r2 = rt * rt
        if not math.isfinite(r2):
            break
        inside = np.nonzero(d2 < r2)[0]
        if len(inside):
            return t, sorted((float(d2[i]), int(i)) for i in inside)
    return UNRESOLVED, []


def blend(cands, C, k):
    """The colour of the k first candidates: the first's at d2 == 0, else the left folds of the header."""
    first = cands[0][0]
    if first == 0.0:
        return tuple(int(x) for x in C[cands[0][1]])
    den = 0.0
    num = [0.0, 0.0, 0.0]
    for d2, i in cands[:k]:
        w = first / d2
        den = den + w
        for c in range(3):
            num[c] = num[c] + w * float(C[i][c])
    out = []
    for c in range(3):
        v = float(np.rint(num[c] / den))  # ties to even
        out.append(int(min(max(v, 0.0), 255.0)))
    return tuple(out)


def transfer_colors(P, C, Q, radius, k=8, max_tiers=None, fill=FILL):
    """-> (out u8 [m, 3] BGR, tier u8 [m]) of the definition in csrc/slmeshcolor.inl."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    C = np.asarray(C, dtype=np.uint8).reshape(-1, 3)
    Q = np.asarray(Q, dtype=np.float64).reshape(-1, 3)
    if len(C) != len(P):
        raise ValueError("colors must have one row of three per point")
    if not (math.isfinite(radius) and radius > 0.0):
        raise ValueError("radius must be finite and > 0")
    if not 1 <= k <= MAX_K:
        raise ValueError("k must be 1..16")
    m = len(Q)
    out = np.empty((m, 3), dtype=np.uint8)
    out[:] = np.asarray(fill, dtype=np.uint8)
    tier = np.full(m, UNRESOLVED, dtype=np.uint8)
    if m == 0 or len(P) == 0:
        return out, tier
    if not np.isfinite(P).all():
        raise ValueError("non-finite cloud coordinates")
    finite = np.isfinite(Q).all(1)
    if not finite.any():
        return out, tier
    last = tier_limit(P, Q, radius)
    if max_tiers is not None:
        last = min(last, int(max_tiers) - 1)
    for j in range(m):
        if not finite[j]:
            continue
        t, cands = candidates(P, Q[j], radius, last)
        if t == UNRESOLVED:
            continue
        tier[j] = t
        out[j] = blend(cands, C, k)
    return out, tier


def mesh_ply_colors_header(n_vertices: int, n_triangles: int) -> bytes:
    return ("ply\nformat binary_little_endian 1.0\ncomment Created by Open3D\n"
            f"element vertex {n_vertices}\n"
            "property double x\nproperty double y\nproperty double z\n"
            "property double nx\nproperty double ny\nproperty double nz\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\n"
            f"element face {n_triangles}\nproperty list uchar uint vertex_indices\nend_header\n").encode("ascii")


def mesh_ply_colors_bytes(vertices, triangles, colors) -> bytes:
    """The coloured binary PLY one record at a time: per vertex six doubles and red green blue from the BGR row."""
    P = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    T = np.asarray(triangles).reshape(-1, 3)
    C = np.asarray(colors, dtype=np.uint8).reshape(-1, 3)
    assert len(C) == len(P)
    VN = vertex_normals(P, T)
    out = [mesh_ply_colors_header(len(P), len(T))]
    for v in range(len(P)):
        b, g, r = (int(x) for x in C[v])
        out.append(struct.pack("<6d3B", *P[v].tolist(), *VN[v].tolist(), r, g, b))
    for t in range(len(T)):
        out.append(struct.pack("<B3I", 3, *(int(i) for i in T[t])))
    return b"".join(out)


def parse_mesh_ply_colors(data: bytes):
    """-> (vertices f64 [V, 3], normals f64 [V, 3], colours BGR u8 [V, 3], triangles int64 [T, 3])."""
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    nv = int(next(ln for ln in lines if ln.startswith("element vertex")).split()[2])
    nt = int(next(ln for ln in lines if ln.startswith("element face")).split()[2])
    assert len(data) == end + 51 * nv + 13 * nt
    rec = np.frombuffer(data, dtype=np.dtype([("pn", "<f8", 6), ("rgb", "u1", 3)]), count=nv, offset=end)
    faces = np.frombuffer(data, dtype=np.dtype([("n", "u1"), ("v", "<u4", 3)]), count=nt, offset=end + 51 * nv)
    assert (faces["n"] == 3).all()
    return (rec["pn"][:, :3].copy(), rec["pn"][:, 3:].copy(), rec["rgb"][:, ::-1].copy(),
            faces["v"].astype(np.int64))


# ---- the cases the CPU and GPU tests share -------------------------------------------------------------------
def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def random_case(n, m, seed=0):
    rng = np.random.default_rng(seed)
    return _ro(rng.random((n, 3)), rng.integers(0, 256, (n, 3), dtype=np.uint8), rng.random((m, 3)))


def two_clusters(seed=5):
    """300 points in the unit cube and 40 in a 0.2 cube at x = 5; 200 queries in the unit cube enlarged by 0.1, 50
    over [0,6]x[0,1]x[0,1], 5 equal to cloud points, one NaN, one at (40, 40, 40).  Radius 0.05."""
    rng = np.random.default_rng(seed)
    P = np.concatenate([rng.random((300, 3)), rng.random((40, 3)) * 0.2 + (5.0, 0.0, 0.0)])
    C = rng.integers(0, 256, (len(P), 3), dtype=np.uint8)
    Q = np.concatenate([rng.random((200, 3)) * 1.2 - 0.1, rng.random((50, 3)) * (6.0, 1.0, 1.0),
                        P[[0, 7, 299, 300, 339]], [[np.nan, 0.5, 0.5]], [[40.0, 40.0, 40.0]]])
    return _ro(P, C, Q) + (0.05,)


def lattice(side=3):
    """The integer lattice 0 .. side - 1 cubed, index = (x side + y) side + z, colours from the index."""
    g = np.arange(side)
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    i = np.arange(len(P))
    C = np.stack([i * 9 % 256, i * 5 % 256, 255 - i * 7 % 256], 1).astype(np.uint8)
    return _ro(P, C)
