"""The CPU restatement of csrc/slmeshwrite.inl that the mesh writers are checked
against: vertex normals as 64-bit fixed-point sums in Python integers, and the
binary PLY of a mesh one record at a time.  The STL side is tests/mesh_oracle.py's
(``triangle_normals``, ``stl_bytes``), imported here, not restated.

Open3D is not installed: its PLY layout (double x y z nx ny nz per vertex, uchar
3 + three uint per face, "comment Created by Open3D") and its rule for a zero
normal sum ((0, 0, 1)) are restated from memory and unpinned.
"""
from __future__ import annotations

import math
import struct

import numpy as np

from tests.mesh_oracle import stl_bytes, triangle_normals  # noqa: F401  (the STL reference, chunk-independent)

VN_FIX = 2.0 ** 40
VN_FIX_MAX = 2.0 ** 62


def _fix(v: float) -> int:
    """llrint(v 2^40) (Python's round: ties to even) for |v 2^40| < 2^62, else 0 (so a NaN adds nothing)."""
    t = v * VN_FIX
    return round(t) if abs(t) < VN_FIX_MAX else 0


def _wrap(s: int) -> int:
    """A Python integer as the int64 a wrapping sum holds."""
    return (s + 2 ** 63) % 2 ** 64 - 2 ** 63


def vertex_normals(vertices, triangles) -> np.ndarray:
    """-> f64 [V, 3]: per vertex the sum over its triangles of _fix(unit normal), as int64; float(sum) (nearest
    even); s / sqrt((sx sx + sy sy) + sz sz), or (0, 0, 1) for three zero sums."""
    P = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    T = np.asarray(triangles).reshape(-1, 3)
    N = triangle_normals(P, T) if len(T) else np.zeros((0, 3))
    sums = [[0, 0, 0] for _ in range(len(P))]
    for t in range(len(T)):
        q = [_fix(float(x)) for x in N[t]]
        for v in T[t]:
            for c in range(3):
                sums[int(v)][c] += q[c]
    out = np.zeros((len(P), 3))
    for v, s in enumerate(sums):
        sx, sy, sz = (float(_wrap(x)) for x in s)
        if sx == 0.0 and sy == 0.0 and sz == 0.0:
            out[v] = (0.0, 0.0, 1.0)
        else:
            ln = math.sqrt((sx * sx + sy * sy) + sz * sz)
            out[v] = (sx / ln, sy / ln, sz / ln)
    return out


def mesh_ply_header(n_vertices: int, n_triangles: int) -> bytes:
    return ("ply\nformat binary_little_endian 1.0\ncomment Created by Open3D\n"
            f"element vertex {n_vertices}\n"
            "property double x\nproperty double y\nproperty double z\n"
            "property double nx\nproperty double ny\nproperty double nz\n"
            f"element face {n_triangles}\nproperty list uchar uint vertex_indices\nend_header\n").encode("ascii")


def mesh_ply_bytes(vertices, triangles) -> bytes:
    """The binary PLY of the mesh with its vertex normals, one record at a time (the slow, obvious way)."""
    P = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    T = np.asarray(triangles).reshape(-1, 3)
    VN = vertex_normals(P, T)
    out = [mesh_ply_header(len(P), len(T))]
    for v in range(len(P)):
        out.append(struct.pack("<6d", *P[v].tolist(), *VN[v].tolist()))
    for t in range(len(T)):
        out.append(struct.pack("<B3I", 3, *(int(i) for i in T[t])))
    return b"".join(out)


def parse_mesh_ply(data: bytes):
    """-> (vertices f64 [V, 3], normals f64 [V, 3], triangles int64 [T, 3]) of a file mesh_ply_bytes lays out."""
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    nv = int(next(ln for ln in lines if ln.startswith("element vertex")).split()[2])
    nt = int(next(ln for ln in lines if ln.startswith("element face")).split()[2])
    assert len(data) == end + 48 * nv + 13 * nt
    vn = np.frombuffer(data, dtype="<f8", count=6 * nv, offset=end).reshape(nv, 6)
    faces = np.frombuffer(data, dtype=np.dtype([("n", "u1"), ("v", "<u4", 3)]), count=nt, offset=end + 48 * nv)
    assert (faces["n"] == 3).all()
    return vn[:, :3].copy(), vn[:, 3:].copy(), faces["v"].astype(np.int64)


# ---- the meshes the CPU and GPU tests share -------------------------------------------------------------------
def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def random_mesh(nt, nv=None, seed=0):
    """nt random triangles over nv (default nt // 2 + 3) random vertices; vertex nv - 1 is in no triangle."""
    nv = nt // 2 + 3 if nv is None else nv
    rng = np.random.default_rng(seed)
    P = rng.normal(size=(nv, 3))
    T = rng.integers(0, max(nv - 1, 1), size=(nt, 3)).astype(np.int32)
    return _ro(P, T)


def degenerate_mesh():
    """A repeated index, three collinear points, three points that coincide (5 + 1e-170 is 5), a cross product that
    underflows to zero (edges of 1e-170), and vertices (0, 1, 2) of two triangles of opposite normals alone, whose
    sums cancel."""
    P = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0],           # 0 1 2 and 0 2 1: opposite normals
                  [2.0, 2.0, 2.0], [3.0, 3.0, 3.0], [4.0, 4.0, 4.0],           # collinear
                  [5.0, 0.0, 0.0], [5.0 + 1e-170, 0.0, 0.0], [5.0, 1e-170, 0.0],  # coincide after rounding
                  [0.0, 0.0, 7.0], [1e-170, 0.0, 7.0], [0.0, 1e-170, 7.0],     # edges 1e-170: the products underflow
                  [1.0, 2.0, 3.0], [-2.0, 0.5, 1.0], [0.25, -1.0, 2.0]])       # an ordinary triangle
    T = np.array([[0, 1, 2], [0, 2, 1], [3, 4, 5], [12, 12, 13], [9, 10, 11], [6, 7, 8], [12, 13, 14]], dtype=np.int32)
    return _ro(P, T)


HALF_EVEN = 1.0 + 2.0 ** -24           # half-way between 1 and 1 + 2^-23: to the even 1.0
HALF_ODD = 1.0 + 3.0 * 2.0 ** -24      # half-way between 1 + 2^-23 and 1 + 2^-22: to the even 1 + 2^-22
CAST_EDGES = (HALF_EVEN, HALF_ODD, 0.0, -0.0, 1e-46, 1e-40, 3.4028235677973366e38, -HALF_EVEN, -1e-40)


def cast_mesh():
    """Vertices whose coordinates are the float32 cast's edges.  Triangles 0-2 keep finite normals (their
    coordinates are the half-way values, the zeros and the tiny ones beside ordinary numbers); triangle 3 has the
    coordinate that rounds to inf, whose f64 normal is still finite (3.4e38 squared is far below the f64 range)."""
    P = np.array([[HALF_EVEN, 0.0, -0.0], [HALF_ODD, 1.0, 1e-46], [-HALF_EVEN, -0.0, 1.0],
                  [1e-40, 2.0, 0.5], [-1e-40, -1.0, 1e-46], [0.5, 1e-40, 3.0],
                  [3.4028235677973366e38, 1.0, 0.0], [0.0, 2.0, 1.0], [1.0, 0.0, 2.0]])
    T = np.array([[0, 1, 2], [3, 4, 5], [0, 4, 2], [6, 7, 8]], dtype=np.int32)
    return _ro(P, T)


def fan_mesh(valence=300):
    """A closed fan of ``valence`` triangles about vertex 0, the rim a bumpy circle: every triangle adds to vertex 0."""
    k = np.arange(valence)
    a = 2.0 * np.pi * k / valence
    rim = np.stack([np.cos(a), np.sin(a), 0.1 * np.sin(7.0 * a)], 1)
    P = np.concatenate([[[0.0, 0.0, 0.5]], rim])
    T = np.stack([np.zeros(valence, np.int64), 1 + k, 1 + (k + 1) % valence], 1).astype(np.int32)
    return _ro(P, T)
