"""Meshing on the GPU: the fourth step of the reference's workflow
(server/processing.py:185-311; ``processing.ProcessingLogic.reconstruct_stl``
and ``mesh_360`` of this package are the drop-ins built on this module):
Poisson reconstruction (mode "watertight") and ball pivoting (mode "surface").

``create_from_point_cloud_poisson`` is Kazhdan's FFT Poisson reconstruction on
a dense periodic grid of R = 2^depth nodes per axis: a trilinear splat of the
oriented points (64-bit fixed-point integer atomics, so the grids do not depend
on the order the points arrive in), the divergence of the splatted normals,
one FFT solve, the iso value as the mean of the field at the points, and
marching tetrahedra over the six Kuhn tetrahedra of every cube.  Everything
but the FFT is a HIP kernel of libslgpu.so (csrc/slmesh.inl, which states the
arithmetic); the FFT is ``torch.fft`` (rocFFT).

``orient_normals_consistent_tangent_plane`` orients estimated normals before
that: the reference's call restated on the kNN graph alone (a minimum spanning
forest over 1 - |ni . nj| by Boruvka rounds, csrc/slorient.inl, checked bit for
bit against tests/orient_oracle.py); the drop-ins use it when asked to
(``tangent_planes=k``).

``create_from_point_cloud_ball_pivoting`` is the reference's other mode
(:220-237).  Open3D's ball pivoting is a sequential front; it is restated in an
order-free form: the triangles with an empty ball of the radius on the side of
their normals are enumerated per point by a HIP kernel (csrc/slbpa.inl, which
states the rules; ``ball_pivot_candidates`` is that enumeration alone), and the
pass bookkeeping -- vertex classes, edge counts, the seed and per-edge rules --
is torch sorts and searches on the device.  tests/bpa_oracle.py is the CPU
restatement the result equals exactly; the triangle set is not Open3D's.

``cluster_connected_triangles``, ``remove_triangles_by_mask``,
``remove_unreferenced_vertices``, ``select_components`` and
``simplify_vertex_clustering`` clean the mesh before it is written: Open3D's
calls of those names in order-free forms (csrc/slmeshclean.inl states them;
tests/meshclean_oracle.py is their CPU form, which the results equal exactly).
The drop-ins apply them when asked to (``keep_largest_component``,
``min_component_triangles``, ``simplify_voxel_size``).

``write_triangle_mesh`` writes the mesh as ``.stl`` or ``.ply``: device tensors
are packed into records by HIP kernels and streamed to the file through a ring
of two pinned chunks (csrc/slmeshwrite.inl states the arithmetic and the
layout); ``compute_triangle_normals`` and ``compute_vertex_normals`` are the
normals it writes (the vertex normals as order-free fixed-point sums; exact
against tests/meshwrite_oracle.py).  ``transfer_colors`` carries a cloud's
colours onto the mesh vertices -- nearest samples by tiers of doubling radius,
an inverse-squared-distance blend (csrc/slmeshcolor.inl states the definition;
exact against tests/meshcolor_oracle.py) -- and ``write_triangle_mesh(...,
colors=...)`` writes them as ``uchar red green blue`` in the ``.ply``.

``filter_smooth_taubin``, ``filter_smooth_laplacian`` and ``filter_smooth_simple``
move the vertices: Open3D's calls of those names on ``adjacency_list``'s CSR
(the sorted sides of the triangles and their transpose), one thread per vertex folding its
neighbours in ascending index (csrc/slmeshsmooth.inl states the rules; exact
against tests/meshsmooth_oracle.py).  The drop-ins apply them when asked to
(``smooth_iterations``, ``smooth_method``, ``smooth_fixed_boundary``).

``check`` says whether a mesh is printable: boundary, non-manifold and
inconsistent edges, non-manifold vertices, orientable, watertight, area and
volume, all from one sort of the triangles' sides (csrc/slmeshcheck.inl states
the definitions; exact against tests/meshcheck_oracle.py).  Open3D's
``is_edge_manifold``, ``is_vertex_manifold``, ``is_orientable``,
``is_watertight``, ``get_non_manifold_edges``, ``get_non_manifold_vertices``,
``get_surface_area`` and ``get_volume`` are views of it, beside
``orient_triangles``, ``remove_degenerate_triangles`` and
``remove_duplicated_triangles``.  The drop-ins report and repair when asked to
(``check_mesh``, ``repair_mesh``).

``fill_holes`` closes the holes ``check`` reports: ``boundary_loops`` lists the
boundary components (sides that share a vertex), and every one that is a plain
cycle within the limits gets a triangle or a fan about its centroid, an
order-free fixed-point mean (csrc/slmeshfill.inl states the definitions; exact
against tests/meshfill_oracle.py).  The drop-ins apply it when asked to
(``fill_holes``, ``fill_hole_size``, ``fill_max_edges``).

Open3D's Poisson is the adaptive-octree variant and is not installed here:
parity with Open3D is unpinned, and tests/mesh_oracle.py is the CPU restatement
the tests check against -- bit for bit for every stage except the solve.
Tensors in and out live on the device; ``origin`` is a NumPy f64 [3].
"""
from __future__ import annotations

import ctypes
import os
import time

import numpy as np
import torch

from . import _lib
from .merge import _call, _engine, _f64, _ptr

_D3 = ctypes.c_double * 3
MAX_DEPTH = 10  # 2^30 nodes: the scans and the kernels' grid sizes are laid out for it


def required_bytes(depth: int, n_points: int) -> int:
    """Device bytes ``create_from_point_cloud_poisson`` needs at its peak, the
    splat: four int64 accumulators and the four f32 grids made from them (48
    bytes a node; every later stage holds less) plus the points, their normals
    and their samples."""
    return 48 * (1 << (3 * int(depth))) + 56 * int(n_points)


def _check_memory(depth, n, dev, budget_bytes):
    need = required_bytes(depth, n)
    if budget_bytes is None:
        free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
    else:
        free = int(budget_bytes)
    if need > free or depth > MAX_DEPTH:
        raise MemoryError(f"Poisson reconstruction at depth {depth} needs {need} bytes of device memory; "
                          f"{free} bytes are available (the largest supported depth is {MAX_DEPTH})")


def _depth_of(grid) -> int:
    R = grid.shape[-1]
    if grid.dtype != torch.float32 or grid.dim() != 3 or tuple(grid.shape) != (R, R, R) or R < 2 or R & (R - 1):
        raise ValueError("a grid must be float32 [R, R, R] with R a power of two")
    return R.bit_length() - 1


def _origin(origin):
    o = np.ascontiguousarray(np.asarray(origin, dtype=np.float64).reshape(3))
    return _D3(*o.tolist())


class _Stages:
    """Milliseconds per stage into ``timings`` (a dict, or None: nothing is measured or synchronised)."""

    def __init__(self, timings, dev):
        self.timings, self.dev = timings, dev
        self.mark(None)

    def mark(self, name):
        if self.timings is None:
            return
        torch.cuda.synchronize(self.dev)
        now = time.perf_counter()
        if name is not None:
            self.timings[name] = self.timings.get(name, 0.0) + (now - self.t0) * 1e3
        self.t0 = now


def box(points, depth: int, scale: float = 1.1):
    """-> (origin f64 [3], h): the cube of side scale * (largest extent) about the points' bounding box."""
    lo = points.min(0).values.cpu().numpy()
    hi = points.max(0).values.cpu().numpy()
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError("points must be finite")
    c = (lo + hi) / 2.0
    L = scale * float((hi - lo).max())
    if not L > 0.0:
        L = 1.0
    if not np.isfinite(L):
        raise ValueError("scale must be finite")
    return c - L / 2.0, L / (1 << depth)


def ordered_sum(values, stride: int = 1, offset: int = 0, *, device=None) -> float:
    """The ordered f64 sum (csrc/slplane.inl) of values[offset::stride]."""
    eng = _engine(device)
    v = torch.as_tensor(values).to(device=eng.device, dtype=torch.float64).contiguous().reshape(-1)
    out = ctypes.c_double()
    _call(eng, "sl_ordered_sum", _ptr(v) if v.numel() else None, v.numel() // stride, stride, offset,
          ctypes.byref(out))
    return out.value


def get_center(points, *, device=None) -> np.ndarray:
    """PointCloud.get_center: the mean of the points (ordered sums) -> NumPy f64 [3]."""
    eng = _engine(device)
    P = _f64(points, eng.device)
    if not len(P):
        return np.zeros(3)
    return np.array([ordered_sum(P, 3, a, device=eng.device) / float(len(P)) for a in range(3)])


def orient_normals_towards_camera_location(points, normals, location=(0.0, 0.0, 0.0), *, device=None):
    """PointCloud.orient_normals_towards_camera_location -> the oriented normals
    (a copy): negated where n . (location - p) < 0; a zero normal becomes the
    unit vector towards the location."""
    eng = _engine(device)
    P = _f64(points, eng.device)
    N = _f64(normals, eng.device).clone()
    if N.shape != P.shape:
        raise ValueError("a normal per point is needed")
    _call(eng, "sl_orient_normals", _ptr(P), _ptr(N), P.shape[0], _origin(location))
    return N


def orient_normals_mst(points, normals, idx, cnt, *, device=None):
    """sl_orient_normals_mst over a given graph (``idx`` int32 [N, k], ``cnt``
    int32 [N], as ``merge.radius_search`` returns them) -> (the oriented normals
    (a copy), {"components", "tree_slots" (int64, ascending), "rounds", "jumps"})."""
    eng = _engine(device)
    P = _f64(points, eng.device)
    N = _f64(normals, eng.device).clone()
    if N.shape != P.shape:
        raise ValueError("a normal per point is needed")
    n = P.shape[0]
    I = torch.as_tensor(idx).to(device=eng.device, dtype=torch.int32).contiguous()
    C = torch.as_tensor(cnt).to(device=eng.device, dtype=torch.int32).contiguous().reshape(-1)
    if I.dim() != 2 or I.shape[0] != n or C.shape[0] != n:
        raise ValueError("the graph needs a row of neighbours and a count per point")
    k = I.shape[1]
    tree = torch.empty(max(n, 1), dtype=torch.int32, device=eng.device)  # slots are uint32
    nt, nc = ctypes.c_int64(), ctypes.c_int64()
    _call(eng, "sl_orient_normals_mst", _ptr(P) if n else None, _ptr(N) if n else None, n,
          _ptr(I) if n and k else None, _ptr(C) if n else None, k, _ptr(tree), ctypes.byref(nt), ctypes.byref(nc))
    rounds, jumps = ctypes.c_int(), (ctypes.c_int * 40)()
    with eng._lock:
        _lib.check(eng._L.sl_orient_normals_mst_stats(ctypes.byref(rounds), jumps, 40), None,
                   "sl_orient_normals_mst_stats")
    slots = torch.sort(tree[: nt.value].to(torch.int64) & 0xFFFFFFFF).values
    return N, {"components": nc.value, "tree_slots": slots, "rounds": rounds.value,
               "jumps": list(jumps[: rounds.value])}


def orient_normals_consistent_tangent_plane(points, normals, k: int = 100, *, radius, device=None, info=False):
    """PointCloud.orient_normals_consistent_tangent_plane(k) -> the oriented
    normals f64 [N, 3] on the device (a copy); with ``info`` also {"components",
    "tree_slots", ...}.  Restated on the kNN graph alone (csrc/slorient.inl
    states the rules): the graph is ``merge.radius_search(points, radius, k)``,
    edges weigh 1 - |ni . nj| and are ordered by (weight, slot), the minimum
    spanning forest propagates the signs, and every connected component is
    rooted at its highest point, whose normal is made to point up.  Open3D adds
    Delaunay-EMST edges, which connect the graph; here a graph of more than one
    component is oriented component by component ("components" tells)."""
    eng = _engine(device)
    P = _f64(points, eng.device)
    N = _f64(normals, eng.device)
    if N.shape != P.shape:
        raise ValueError("a normal per point is needed")
    from . import merge
    idx, _, cnt = merge.radius_search(P, radius, int(k), device=eng.device)
    out, inf = orient_normals_mst(P, N, idx, cnt, device=eng.device)
    return (out, inf) if info else out


def sample(grid, points, origin, h, *, device=None) -> torch.Tensor:
    """Trilinear value (f64) of a float32 [R, R, R] grid at every point."""
    eng = _engine(device)
    G = torch.as_tensor(grid).to(eng.device).contiguous()
    depth = _depth_of(G)
    P = _f64(points, eng.device)
    out = torch.empty(max(len(P), 1), dtype=torch.float64, device=eng.device)
    _call(eng, "sl_mesh_sample", _ptr(G), depth, _origin(origin), float(h), _ptr(P), P.shape[0], _ptr(out))
    return out[: len(P)]


def vertex_density(W, vertices, origin, h, *, device=None) -> torch.Tensor:
    """The density of every vertex: the splatted weight W at its position."""
    return sample(W, vertices, origin, h, device=device)


def solve(div, h) -> torch.Tensor:
    """chi = irfftn(rfftn(div) / lambda), lambda the 7-point Laplacian's eigenvalues, chi^(0) = 0 (float32)."""
    R = div.shape[0]
    c = torch.from_numpy((2.0 * np.cos(2.0 * np.pi * np.arange(R) / R) - 2.0).astype(np.float32)).to(div.device)
    F = torch.fft.rfftn(div)
    lam = (c[:, None, None] + c[None, :, None]) + c[None, None, : R // 2 + 1]
    lam /= float(np.float32(h * h))
    lam[0, 0, 0] = 1.0
    F /= lam
    del lam
    F[0, 0, 0] = 0.0
    return torch.fft.irfftn(F, s=tuple(div.shape)).contiguous()


def poisson_field(points, normals, depth: int, scale: float = 1.1, *, keep: bool = False, budget_bytes=None,
                  timings=None, device=None) -> dict:
    """Splat, divergence, solve and iso value -> {"chi", "W" (float32 [R, R, R]),
    "iso", "origin", "h"}; with ``keep`` also "V" (float32 [3, R, R, R]) and
    "div".  ``budget_bytes`` replaces the device's free memory in the check
    that raises MemoryError before anything is allocated; ``timings`` (a dict)
    receives the milliseconds of each stage."""
    eng = _engine(device)
    P = _f64(points, eng.device)
    N = _f64(normals, eng.device)
    if N.shape != P.shape:
        raise ValueError("a normal per point is needed")
    n = P.shape[0]
    if n == 0:
        raise ValueError("no points")
    depth = int(depth)
    if depth < 1:
        raise ValueError("depth must be at least 1")
    _check_memory(depth, n, eng.device, budget_bytes)
    R = 1 << depth
    st = _Stages(timings, eng.device)
    origin, h = box(P, depth, scale)
    o = _origin(origin)
    acc = torch.zeros((4, R, R, R), dtype=torch.int64, device=eng.device)
    _call(eng, "sl_mesh_splat", _ptr(P), _ptr(N), n, depth, o, h, _ptr(acc))
    G = torch.empty((4, R, R, R), dtype=torch.float32, device=eng.device)
    _call(eng, "sl_mesh_unfix", _ptr(acc), acc.numel(), _ptr(G))
    del acc  # the accumulators are gone before the FFT
    st.mark("splat")
    W = G[0].clone()
    V = G[1:]
    div = torch.empty((R, R, R), dtype=torch.float32, device=eng.device)
    _call(eng, "sl_mesh_divergence", _ptr(V), depth, h, _ptr(div))
    out = {"W": W, "origin": origin, "h": h}
    if keep:
        out["V"] = V.clone()
        out["div"] = div.clone()
    del G, V
    st.mark("divergence")
    chi = solve(div, h)
    del div
    st.mark("solve")
    out["chi"] = chi
    out["iso"] = iso_value(chi, P, origin, h, device=eng.device)
    st.mark("iso")
    return out


def iso_value(chi, points, origin, h, *, device=None) -> float:
    """The mean of chi at the points (ordered sum)."""
    s = sample(chi, points, origin, h, device=device)
    return ordered_sum(s, device=s.device) / float(len(s))


def extract_isosurface(chi, iso: float, origin, h, *, device=None):
    """Marching tetrahedra -> (vertices f64 [V, 3], triangles int32 [T, 3]);
    triangles are wound so that the normal points to the chi > iso side."""
    eng = _engine(device)
    chi = torch.as_tensor(chi).to(eng.device).contiguous()
    depth = _depth_of(chi)
    n3 = chi.numel()
    o = _origin(origin)
    emask = torch.empty(n3, dtype=torch.uint8, device=eng.device)
    vpos = torch.empty(n3, dtype=torch.int32, device=eng.device)
    tpos = torch.empty(n3, dtype=torch.int32, device=eng.device)
    nv, nt = ctypes.c_int64(), ctypes.c_int64()
    _call(eng, "sl_mesh_extract_count", _ptr(chi), depth, float(iso), _ptr(emask), _ptr(vpos), _ptr(tpos),
          ctypes.byref(nv), ctypes.byref(nt))
    verts = torch.empty((max(nv.value, 1), 3), dtype=torch.float64, device=eng.device)
    tris = torch.empty((max(nt.value, 1), 3), dtype=torch.int32, device=eng.device)
    _call(eng, "sl_mesh_extract_emit", _ptr(chi), depth, float(iso), o, float(h), _ptr(emask), _ptr(vpos),
          _ptr(tpos), nv.value, nt.value, _ptr(verts), _ptr(tris))
    return verts[: nv.value], tris[: nt.value]


def remove_vertices_by_mask(vertices, triangles, mask, *, device=None):
    """TriangleMesh.remove_vertices_by_mask -> (vertices, triangles): the masked
    vertices and every triangle that has one go; the rest keep their order."""
    eng = _engine(device)
    Vx = _f64(vertices, eng.device)
    T = torch.as_tensor(triangles).to(device=eng.device, dtype=torch.int32).contiguous().reshape(-1, 3)
    M = torch.as_tensor(mask).to(device=eng.device).reshape(-1).ne(0).to(torch.uint8).contiguous()
    if len(M) != len(Vx):
        raise ValueError("a mask entry per vertex is needed")
    ov = torch.empty((max(len(Vx), 1), 3), dtype=torch.float64, device=eng.device)
    ot = torch.empty((max(len(T), 1), 3), dtype=torch.int32, device=eng.device)
    nv, nt = ctypes.c_int64(), ctypes.c_int64()
    _call(eng, "sl_mesh_remove_vertices", _ptr(Vx), len(Vx), _ptr(T), len(T), _ptr(M), _ptr(ov), _ptr(ot),
          ctypes.byref(nv), ctypes.byref(nt))
    return ov[: nv.value], ot[: nt.value]


def _tris(triangles, dev) -> torch.Tensor:
    T = torch.as_tensor(triangles)
    if T.numel() and (T.dim() != 2 or T.shape[1] != 3):
        raise ValueError("triangles must be (T, 3)")
    return T.to(device=dev, dtype=torch.int32).contiguous().reshape(-1, 3)


def cluster_connected_triangles(vertices, triangles, *, n_vertices=None, area=True, device=None):
    """TriangleMesh.cluster_connected_triangles -> (triangle_clusters int32 [T],
    cluster_n_triangles int64 [C], cluster_area f64 [C] | None) on the device.
    Two triangles are adjacent iff they share an edge (a shared vertex alone
    does not connect); a cluster is a connected component and its label the
    rank of its smallest triangle index, which is what Open3D's breadth-first
    loop assigns (csrc/slmeshclean.inl states the rules, tests/meshclean_oracle.py
    is their CPU form, which the result equals exactly).  The areas need the
    vertices; labels and counts do not: ``vertices`` may be None when
    ``n_vertices`` is given, and then (or with ``area=False``) no area is
    computed and the sort by label it needs is not run.  Deviation: a cluster's
    area is summed in ascending triangle index in blocks of 64 (Open3D: in
    breadth-first order), so the last bits can differ.  An index outside
    0 .. V - 1 raises IndexError."""
    eng, Vx, T, nv = _check_args(vertices, triangles, n_vertices, device)
    t = len(T)
    want = bool(area) and Vx is not None
    labels = torch.empty(max(t, 1), dtype=torch.int32, device=eng.device)
    counts = torch.empty(max(t, 1), dtype=torch.int64, device=eng.device)
    areas = torch.empty(max(t, 1), dtype=torch.float64, device=eng.device) if want else None
    nc = ctypes.c_int64()
    _call(eng, "sl_mesh_cluster_triangles", _ptr(Vx) if Vx is not None and len(Vx) else None, nv,
          _ptr(T) if t else None, t, _ptr(labels), _ptr(counts), _ptr(areas), ctypes.byref(nc))
    return labels[:t], counts[: nc.value], (areas[: nc.value] if want else None)


def _stats(device, symbol, n) -> list:
    """The n doubles that this thread's last call left with the library's ``symbol(double*, int)``."""
    v = (ctypes.c_double * n)()
    _lib.check(getattr(_engine(device)._L, symbol)(v, n), None, symbol)
    return list(v)


def _stage_ms(device, symbol, names) -> dict:
    """``_stats`` under ``names``, in order: host milliseconds per stage."""
    return dict(zip(names, _stats(device, symbol, len(names))))


def cluster_stats(*, device=None) -> dict:
    """Host milliseconds per stage of this thread's last ``cluster_connected_triangles``
    (sl_mesh_cluster_triangles_stats; a measurement aid)."""
    return _stage_ms(device, "sl_mesh_cluster_triangles_stats",
                     ("edge_keys_ms", "sort_ms", "union_ms", "flatten_rank_ms", "counts_ms", "areas_ms"))


def remove_triangles_by_mask(vertices, triangles, mask, *, device=None):
    """TriangleMesh.remove_triangles_by_mask -> (vertices, triangles): the
    masked triangles go and the rest keep their order; the vertices are
    untouched, as in Open3D."""
    eng = _engine(device)
    Vx = _f64(vertices, eng.device)
    T = _tris(triangles, eng.device)
    M = torch.as_tensor(mask).to(device=eng.device).reshape(-1).ne(0).to(torch.uint8).contiguous()
    if len(M) != len(T):
        raise ValueError("a mask entry per triangle is needed")
    out = torch.empty((max(len(T), 1), 3), dtype=torch.int32, device=eng.device)
    nt = ctypes.c_int64()
    _call(eng, "sl_mesh_remove_triangles", _ptr(T) if len(T) else None, len(T), _ptr(M), _ptr(out), ctypes.byref(nt))
    return Vx, out[: nt.value]


def remove_unreferenced_vertices(vertices, triangles, *, device=None):
    """TriangleMesh.remove_unreferenced_vertices -> (vertices, triangles): the
    vertices of no triangle go, the rest keep their order, and the triangles
    are re-indexed.  An index outside 0 .. V - 1 raises IndexError."""
    eng = _engine(device)
    Vx = _f64(vertices, eng.device)
    T = _tris(triangles, eng.device)
    ov = torch.empty((max(len(Vx), 1), 3), dtype=torch.float64, device=eng.device)
    ot = torch.empty((max(len(T), 1), 3), dtype=torch.int32, device=eng.device)
    nv = ctypes.c_int64()
    _call(eng, "sl_mesh_remove_unreferenced", _ptr(Vx) if len(Vx) else None, len(Vx), _ptr(T) if len(T) else None,
          len(T), _ptr(ov), _ptr(ot), ctypes.byref(nv))
    return ov[: nv.value], ot[: len(T)]


def select_components(vertices, triangles, *, keep_largest: bool = False, min_triangles=None, device=None):
    """cluster_connected_triangles + remove_triangles_by_mask +
    remove_unreferenced_vertices -> (vertices, triangles): ``min_triangles``
    first drops the clusters with fewer triangles, then ``keep_largest`` keeps
    the remaining cluster with the most triangles (the lowest label on a tie),
    then the unreferenced vertices are removed."""
    eng = _engine(device)
    Vx = _f64(vertices, eng.device)
    T = _tris(triangles, eng.device)
    labels, counts, _ = cluster_connected_triangles(Vx, T, area=False, device=eng.device)
    keep = torch.ones(len(counts), dtype=torch.bool, device=eng.device)
    if min_triangles is not None:
        keep &= counts >= int(min_triangles)
    if keep_largest and bool(keep.any()):
        c = torch.where(keep, counts, torch.full_like(counts, -1))
        first = torch.nonzero(c == c.max())[0, 0]  # the lowest label on a tie
        keep = torch.zeros_like(keep)
        keep[first] = True
    mask = ~keep[labels.to(torch.int64)]
    _, T = remove_triangles_by_mask(Vx, T, mask, device=eng.device)
    return remove_unreferenced_vertices(Vx, T, device=eng.device)


def simplify_vertex_clustering(vertices, triangles, voxel_size: float, *, device=None):
    """TriangleMesh.simplify_vertex_clustering(voxel_size, contraction=Average)
    -> (vertices f64 [V', 3], triangles int32 [T', 3]) on the device.  The grid
    is ``merge.voxel_down_sample``'s over all vertices, referenced or not
    (lo = min - voxel_size / 2; its limits and messages).  A voxel's new index
    is the rank of its smallest member vertex index (Open3D's first-encounter
    numbering) and its vertex the members' mean, summed in ascending vertex
    index.  Triangles, in input order: mapped, dropped when two indices are
    equal, rotated so that the smallest index comes first (the orientation is
    kept; the opposite orientation is another triple), the first occurrence of
    every triple kept.  Deviations: Open3D sums a voxel's members and emits the
    triangles in the order of an unordered_set; here both orders are fixed (the
    last bits of a vertex can differ, and the triangles come in input order of
    their first occurrences).  The result is in general NOT manifold -- edges
    with more than two triangles and holes appear where the surface is thinner
    than a voxel; that is the algorithm, and nothing repairs it.  A non-finite
    vertex raises ValueError, an index outside 0 .. V - 1 IndexError."""
    eng = _engine(device)
    Vx = _f64(vertices, eng.device)
    T = _tris(triangles, eng.device)
    ov = torch.empty((max(len(Vx), 1), 3), dtype=torch.float64, device=eng.device)
    ot = torch.empty((max(len(T), 1), 3), dtype=torch.int32, device=eng.device)
    nv, nt = ctypes.c_int64(), ctypes.c_int64()
    _call(eng, "sl_mesh_simplify_clustering", _ptr(Vx) if len(Vx) else None, len(Vx), _ptr(T) if len(T) else None,
          len(T), float(voxel_size), _ptr(ov), _ptr(ot), ctypes.byref(nv), ctypes.byref(nt))
    return ov[: nv.value], ot[: nt.value]


def adjacency_list(triangles, n_vertices, *, boundary: bool = False, device=None):
    """TriangleMesh.compute_adjacency_list as CSR -> (row_start int64 [V + 1],
    neighbours int32 [M][, boundary bool [V]]) on the device: row v, the indices
    that share a triangle with v, is ``neighbours[row_start[v]:row_start[v + 1]]``,
    ascending without duplicates; a vertex of no triangle has an empty row.  As
    in Open3D's inserts a triangle that repeats an index puts the vertex into its
    own set: (a, a, b) gives N(a) = {a, b}.  ``boundary``: also the vertices with
    an edge {v, w}, w != v, that is the side of exactly one triangle
    (csrc/slmeshsmooth.inl states the rules, tests/meshsmooth_oracle.py is their
    CPU form, which the result equals exactly).  An index outside 0 .. V - 1
    raises IndexError."""
    eng = _engine(device)
    T = _tris(triangles, eng.device)
    nv, t = int(n_vertices), len(T)
    if not 0 <= nv < 2 ** 31:
        raise ValueError("n_vertices must be in 0 .. 2^31 - 1")
    rows = torch.empty(nv + 1, dtype=torch.int64, device=eng.device)
    nb = torch.empty(max(6 * t, 1), dtype=torch.int32, device=eng.device)
    bnd = torch.empty(max(nv, 1), dtype=torch.uint8, device=eng.device) if boundary else None
    m = ctypes.c_int64()
    _call(eng, "sl_mesh_adjacency", _ptr(T) if t else None, t, nv, _ptr(rows), _ptr(nb), _ptr(bnd), ctypes.byref(m))
    nb = nb[: m.value].clone()  # (not a view of the 6 T capacity)
    return (rows, nb, bnd[:nv].bool()) if boundary else (rows, nb)


_SMOOTH_METHODS = {"simple": 0, "laplacian": 1, "taubin": 2}


def _smooth(method, vertices, triangles, iterations, lam, mu, fixed_boundary, device):
    eng, V, T = _mesh_args(vertices, triangles, device)
    if int(iterations) != iterations or iterations < 0:
        raise ValueError("iterations must be a non-negative integer")
    if not (np.isfinite(lam) and np.isfinite(mu)):
        raise ValueError("lambda_filter and mu must be finite")
    out = torch.empty((max(len(V), 1), 3), dtype=torch.float64, device=eng.device)
    _call(eng, "sl_mesh_smooth", _ptr(V) if len(V) else None, len(V), _ptr(T) if len(T) else None, len(T),
          _SMOOTH_METHODS[method], int(iterations), float(lam), float(mu), int(bool(fixed_boundary)), _ptr(out))
    return out[: len(V)]


def filter_smooth_simple(vertices, triangles, iterations: int = 1, *, fixed_boundary: bool = False, device=None):
    """TriangleMesh.filter_smooth_simple -> the new vertices f64 [V, 3] on the
    device (the triangles are untouched): per iteration and axis, p' = (p + the
    neighbours' p in ascending index) / (1 + |N(v)|), every step from the previous
    step's positions; ``iterations = 0`` returns a copy.  Deviations: Open3D
    walks an unordered_set, so its last bits depend on the hash order, here the
    sum runs in ascending neighbour index (``adjacency_list``'s rows); with
    ``fixed_boundary`` (an extension; off is Open3D's behaviour) the boundary
    vertices keep their position in every step and their neighbours still read
    them.  Only the vertices are filtered, not normals or colours.  Exact against
    tests/meshsmooth_oracle.py (csrc/slmeshsmooth.inl states the rules).  A
    non-finite vertex or negative ``iterations`` raises ValueError, an index
    outside 0 .. V - 1 IndexError."""
    return _smooth("simple", vertices, triangles, iterations, 0.0, 0.0, fixed_boundary, device)


def filter_smooth_laplacian(vertices, triangles, iterations: int = 1, lambda_filter: float = 0.5, *,
                            fixed_boundary: bool = False, device=None):
    """TriangleMesh.filter_smooth_laplacian -> the new vertices f64 [V, 3] on the
    device: ``iterations`` steps p' = p + lambda (sum_j w_j p_j / sum_j w_j - p)
    with w_j = 1 / (|p - p_j| + 1e-12) over the neighbours in ascending index,
    every step from the previous step's positions.  Deviations: the fold order
    (Open3D: the order of an unordered_set); a vertex of no triangle keeps its
    position (Open3D divides 0 / 0); ``fixed_boundary`` as in
    ``filter_smooth_simple``.  A non-finite vertex or ``lambda_filter`` or
    negative ``iterations`` raises ValueError, an index outside 0 .. V - 1
    IndexError."""
    return _smooth("laplacian", vertices, triangles, iterations, lambda_filter, 0.0, fixed_boundary, device)


def filter_smooth_taubin(vertices, triangles, iterations: int = 1, lambda_filter: float = 0.5, mu: float = -0.53, *,
                         fixed_boundary: bool = False, device=None):
    """TriangleMesh.filter_smooth_taubin -> the new vertices f64 [V, 3] on the
    device: per iteration ``filter_smooth_laplacian``'s step with factor
    ``lambda_filter`` and then with ``mu`` (negative: it undoes the shrinkage of
    the first), 2 x iterations launches.  The same deviations and errors; ``mu``
    must be finite too."""
    return _smooth("taubin", vertices, triangles, iterations, lambda_filter, mu, fixed_boundary, device)


def smooth_stats(*, device=None) -> dict:
    """Host milliseconds per stage of this thread's last ``adjacency_list`` or
    ``filter_smooth_*`` (sl_mesh_smooth_stats; a measurement aid)."""
    return _stage_ms(device, "sl_mesh_smooth_stats", ("keys_ms", "sort_ms", "csr_ms", "iterations_ms"))


def _check_args(vertices, triangles, n_vertices, device):
    """-> (engine, vertices f64 | None, triangles int32, V): ``vertices`` may be None when ``n_vertices`` is given."""
    eng = _engine(device)
    Vx = None if vertices is None else _f64(vertices, eng.device)
    if Vx is None and n_vertices is None:
        raise ValueError("vertices or n_vertices is needed")
    nv = len(Vx) if n_vertices is None else int(n_vertices)
    if Vx is not None and nv != len(Vx):
        raise ValueError("n_vertices does not match the vertices")
    if not 0 <= nv < 2 ** 31:
        raise ValueError("n_vertices must be in 0 .. 2^31 - 1")
    return eng, Vx, _tris(triangles, eng.device), nv


def _mesh_check(eng, T, nv, *, allow_boundary_edges=True, edges=False, vertices=False, orient=False) -> dict:
    """One sl_mesh_check -> the counts and booleans, plus the lists that were asked for."""
    t, dev = len(T), eng.device
    allow = bool(allow_boundary_edges)
    counts = (ctypes.c_int64 * 8)()
    E = torch.empty((max((1 if allow else 3) * t, 1), 2), dtype=torch.int32, device=dev) if edges else None
    L = torch.empty(max(nv, 1), dtype=torch.int32, device=dev) if vertices else None
    O = torch.empty((max(t, 1), 3), dtype=torch.int32, device=dev) if orient else None
    _call(eng, "sl_mesh_check", _ptr(T) if t else None, t, nv, int(allow), counts, _ptr(E), _ptr(L), _ptr(O))
    c = {"vertices": nv, "triangles": t, "edges": counts[0], "boundary_edges": counts[1],
         "non_manifold_edges": counts[2], "inconsistent_edges": counts[3], "non_manifold_vertices": counts[4],
         "degenerate_triangles": counts[5]}
    c["edge_manifold"] = counts[2] == 0
    c["edge_manifold_closed"] = counts[2] == 0 and counts[1] == 0
    c["vertex_manifold"] = counts[4] == 0
    c["orientable"] = counts[6] != 0
    c["consistent"] = counts[3] == 0
    c["watertight"] = c["edge_manifold_closed"] and c["vertex_manifold"] and c["consistent"]
    if edges:
        c["edge_list"] = E[: counts[7]].clone()      # (not views of the capacities)
    if vertices:
        c["vertex_list"] = L[: counts[4]].clone()
    if orient:
        c["oriented"] = O[:t]
    return c


def _measure(eng, Vx, T):
    """sl_mesh_measure -> (area, signed volume): the ordered sums of A_t and W_t in triangle order."""
    a, w = ctypes.c_double(), ctypes.c_double()
    _call(eng, "sl_mesh_measure", _ptr(Vx) if len(Vx) else None, len(Vx), _ptr(T) if len(T) else None, len(T),
          ctypes.byref(a), ctypes.byref(w))
    return a.value, w.value


def check(vertices, triangles, *, n_vertices=None, device=None) -> dict:
    """Everything the mesh checks know about a mesh, from one sort of its sides
    (csrc/slmeshcheck.inl states the definitions; exact against
    tests/meshcheck_oracle.py) -> a dict: the counts "vertices", "triangles",
    "edges" (distinct), "boundary_edges" (one side), "non_manifold_edges" (three
    or more sides), "inconsistent_edges" (two sides of the same direction),
    "non_manifold_vertices" and "degenerate_triangles"; the booleans
    "edge_manifold" (no non-manifold edge), "edge_manifold_closed" (and no
    boundary edge), "vertex_manifold", "orientable", "consistent" (no
    inconsistent edge) and "watertight" (closed, vertex-manifold and consistent,
    as given); "area", and "volume" / "signed_volume" where they are defined (a
    watertight mesh; positive signed volume: the windings face outward), else
    None.  ``vertices`` may be None when ``n_vertices`` is given: the measures
    are None then.  A degenerate triangle (two equal indices) gives its sides to
    the edge counts and takes no part in the vertex test.  An index outside
    0 .. V - 1 raises IndexError, a non-finite vertex ValueError."""
    eng, Vx, T, nv = _check_args(vertices, triangles, n_vertices, device)
    c = _mesh_check(eng, T, nv)
    c["area"] = c["volume"] = c["signed_volume"] = None
    if Vx is not None:
        c["area"], w = _measure(eng, Vx, T)
        if c["watertight"]:
            c["volume"], c["signed_volume"] = abs(w), w
    return c


def check_stats(*, device=None) -> dict:
    """Host milliseconds per stage of this thread's last mesh check or measure
    (sl_mesh_check_stats; a measurement aid)."""
    return _stage_ms(device, "sl_mesh_check_stats",
                     ("side_keys_ms", "sort_ms", "classify_ms", "corners_ms", "parity_ms", "flips_ms", "measure_ms"))


def get_non_manifold_edges(vertices, triangles, allow_boundary_edges: bool = True, *, n_vertices=None, device=None):
    """TriangleMesh.get_non_manifold_edges -> int32 [E, 2] on the device: the
    edges with three or more sides, and with ``allow_boundary_edges=False`` those
    with one side too, as rows (min, max) in ascending order of min V + max.
    Deviation: Open3D returns the order of a hash map."""
    eng, _, T, nv = _check_args(vertices, triangles, n_vertices, device)
    return _mesh_check(eng, T, nv, allow_boundary_edges=allow_boundary_edges, edges=True)["edge_list"]


def get_non_manifold_vertices(vertices, triangles, *, n_vertices=None, device=None):
    """TriangleMesh.get_non_manifold_vertices -> int32 [M] on the device,
    ascending: the vertices whose corners fall into more than one class (two
    corners at a vertex are joined iff their triangles share an edge that
    contains it).  Deviation: degenerate triangles take no part."""
    eng, _, T, nv = _check_args(vertices, triangles, n_vertices, device)
    return _mesh_check(eng, T, nv, vertices=True)["vertex_list"]


def is_edge_manifold(vertices, triangles, allow_boundary_edges: bool = True, *, n_vertices=None, device=None) -> bool:
    """TriangleMesh.is_edge_manifold: no edge with three or more sides, and with
    ``allow_boundary_edges=False`` none with one side either."""
    eng, _, T, nv = _check_args(vertices, triangles, n_vertices, device)
    c = _mesh_check(eng, T, nv)
    return c["edge_manifold"] if allow_boundary_edges else c["edge_manifold_closed"]


def is_vertex_manifold(vertices, triangles, *, n_vertices=None, device=None) -> bool:
    """TriangleMesh.is_vertex_manifold: ``get_non_manifold_vertices`` is empty."""
    eng, _, T, nv = _check_args(vertices, triangles, n_vertices, device)
    return _mesh_check(eng, T, nv)["vertex_manifold"]


def is_orientable(vertices, triangles, *, n_vertices=None, device=None) -> bool:
    """TriangleMesh.is_orientable: no edge has three or more sides and some
    choice of flipped triangles makes every two-sided edge consistent."""
    eng, _, T, nv = _check_args(vertices, triangles, n_vertices, device)
    return _mesh_check(eng, T, nv)["orientable"]


def is_watertight(vertices, triangles, *, check_self_intersection: bool = False, n_vertices=None,
                  device=None) -> bool:
    """TriangleMesh.is_watertight without its self-intersection test: edge-manifold
    with no boundary, vertex-manifold and no inconsistent edge, as given (no
    flips are searched).  Deviation: Open3D also rejects self-intersecting
    meshes (an O(T^2) triangle-pair loop); ``check_self_intersection=True``
    raises NotImplementedError."""
    if check_self_intersection:
        raise NotImplementedError("the self-intersection test of is_watertight is not provided")
    eng, _, T, nv = _check_args(vertices, triangles, n_vertices, device)
    return _mesh_check(eng, T, nv)["watertight"]


def orient_triangles(vertices, triangles, *, n_vertices=None, device=None):
    """TriangleMesh.orient_triangles -> (triangles int32 [T, 3] on the device,
    orientable).  Components are connected through two-sided edges; in each the
    smallest triangle index keeps its winding and a flipped (a, b, c) becomes
    (a, c, b).  Deviations: Open3D seeds a component from an unordered_set; when
    the mesh is not orientable the triangles come back unchanged (Open3D leaves
    them half flipped).  The input is never modified."""
    eng, _, T, nv = _check_args(vertices, triangles, n_vertices, device)
    c = _mesh_check(eng, T, nv, orient=True)
    return c["oriented"], c["orientable"]


def get_surface_area(vertices, triangles, *, device=None) -> float:
    """TriangleMesh.get_surface_area: the ordered sum (``ordered_sum``) of the
    triangles' areas in triangle order."""
    eng, Vx, T, _ = _check_args(vertices, triangles, None, device)
    return _measure(eng, Vx, T)[0]


def get_volume(vertices, triangles, *, signed: bool = False, device=None) -> float:
    """TriangleMesh.get_volume: |the ordered sum of the tetrahedra (0, v0, v1, v2)|;
    with ``signed`` (an extension) the sum itself, positive iff the windings
    face outward.  A mesh that is not watertight (``is_watertight``) raises
    ValueError, as Open3D throws."""
    eng, Vx, T, nv = _check_args(vertices, triangles, None, device)
    if not _mesh_check(eng, T, nv)["watertight"]:
        raise ValueError("The mesh is not watertight, and the volume cannot be computed.")
    w = _measure(eng, Vx, T)[1]
    return w if signed else abs(w)


def _remove(name, vertices, triangles, n_vertices, device):
    eng, Vx, T, nv = _check_args(vertices, triangles, n_vertices, device)
    out = torch.empty((max(len(T), 1), 3), dtype=torch.int32, device=eng.device)
    nt = ctypes.c_int64()
    _call(eng, name, _ptr(T) if len(T) else None, len(T), nv, _ptr(out), ctypes.byref(nt))
    return Vx, out[: nt.value]


def remove_degenerate_triangles(vertices, triangles, *, n_vertices=None, device=None):
    """TriangleMesh.remove_degenerate_triangles -> (vertices, triangles): the
    triangles with two equal indices go, the rest keep their order; the
    vertices are untouched."""
    return _remove("sl_mesh_remove_degenerate", vertices, triangles, n_vertices, device)


def remove_duplicated_triangles(vertices, triangles, *, n_vertices=None, device=None):
    """TriangleMesh.remove_duplicated_triangles -> (vertices, triangles): two
    triangles are the same iff their triples are equal after a rotation that puts
    the strictly smallest index first (the opposite winding is another
    triangle); the first occurrence of each is kept, in input order --
    ``simplify_vertex_clustering``'s rule.  Deviation: the kept triangle is
    stored as it was given (Open3D stores the rotated form)."""
    return _remove("sl_mesh_remove_duplicated_triangles", vertices, triangles, n_vertices, device)


_FILL_COUNTS = ("components", "simple_loops", "filled", "skipped_not_simple", "skipped_by_limit", "new_vertices",
                "new_triangles", "boundary_sides")


def boundary_loops(vertices, triangles, *, n_vertices=None, device=None) -> dict:
    """The boundary components of a mesh (csrc/slmeshfill.inl states the
    definitions; exact against tests/meshfill_oracle.py) -> a dict of device
    tensors with one row per component, in ascending label: "label" int32 (the
    component's smallest vertex), "size" int64 (its boundary sides), "simple"
    bool (every vertex has one side leaving and one entering: one cycle, which
    ``fill_holes`` can close), and "extent" f64 (the diagonal of the box of its
    vertices) when ``vertices`` is given.  A boundary side is a triangle side
    whose edge no other side shares; sides that share an end vertex are one
    component.  ``vertices`` may be None when ``n_vertices`` is given."""
    eng, Vx, T, nv = _check_args(vertices, triangles, n_vertices, device)
    dev, t = eng.device, len(T)
    counts = (ctypes.c_int64 * 8)()
    args = (_ptr(T) if t else None, t, _ptr(Vx) if Vx is not None and nv else None, nv)
    _call(eng, "sl_mesh_boundary_loops", *args, None, None, None, None, counts)      # the number of rows
    rows = counts[0]
    out = {"label": torch.empty(rows, dtype=torch.int32, device=dev),
           "size": torch.empty(rows, dtype=torch.int64, device=dev),
           "simple": torch.empty(rows, dtype=torch.uint8, device=dev)}
    if Vx is not None:
        out["extent"] = torch.empty(rows, dtype=torch.float64, device=dev)
    if rows:
        _call(eng, "sl_mesh_boundary_loops", *args, _ptr(out["label"]), _ptr(out["size"]), _ptr(out["simple"]),
              _ptr(out.get("extent")), counts)
    out["simple"] = out["simple"].to(torch.bool)
    return out


def fill_holes(vertices, triangles, *, hole_size=None, max_hole_edges=None, info: bool = False, device=None):
    """Close the holes of a mesh that are plain loops -> (vertices f64 [V', 3],
    triangles int32 [T', 3]) on the device, and with ``info`` the counts dict
    too (csrc/slmeshfill.inl states the definitions; exact against
    tests/meshfill_oracle.py).  A simple loop (``boundary_loops``) of three
    sides a -> b -> c -> a gets the triangle (a, c, b); a longer one gets one new
    vertex at its centroid and the triangle (b, a, centre) per side a -> b, so
    a consistently wound mesh stays consistent.  ``max_hole_edges`` and
    ``hole_size`` (the largest extent, inclusive) leave larger loops open.
    Components that are not simple loops -- holes that touch in a vertex, the
    open fans at a non-manifold vertex -- are skipped and counted.  The old
    vertices and triangles are a prefix of the results; the new vertices follow
    in ascending label, the new triangles in ascending from-vertex.  Counts:
    "components", "simple_loops", "filled", "skipped_not_simple",
    "skipped_by_limit", "new_vertices", "new_triangles", "boundary_sides".
    Deviations: centroid fans, not a minimal-area triangulation; parity with
    Open3D's fill_holes is unpinned.  A negative or NaN limit raises ValueError.
    The inputs are never modified."""
    if hole_size is not None and not float(hole_size) >= 0.0:
        raise ValueError("hole_size must be a number >= 0")
    if max_hole_edges is not None and int(max_hole_edges) < 0:
        raise ValueError("max_hole_edges must be >= 0")
    eng, Vx, T, nv = _check_args(vertices, triangles, None, device)
    dev, t = eng.device, len(T)
    counts = (ctypes.c_int64 * 8)()
    args = (_ptr(Vx) if nv else None, nv, _ptr(T) if t else None, t,
            -1 if max_hole_edges is None else int(max_hole_edges), -1.0 if hole_size is None else float(hole_size))
    _call(eng, "sl_mesh_fill_holes", *args, None, None, counts)                       # the sizes of the results
    Vo = torch.empty((nv + counts[5], 3), dtype=torch.float64, device=dev)
    To = torch.empty((t + counts[6], 3), dtype=torch.int32, device=dev)
    if counts[6]:
        _call(eng, "sl_mesh_fill_holes", *args, _ptr(Vo), _ptr(To), counts)
    else:
        Vo.copy_(Vx)
        To.copy_(T)
    return (Vo, To, dict(zip(_FILL_COUNTS, counts))) if info else (Vo, To)


def fill_stats(*, device=None) -> dict:
    """Host milliseconds per stage of this thread's last ``fill_holes`` or
    ``boundary_loops`` call into the library (sl_mesh_fill_stats; a measurement
    aid; both make two calls, the first of which only counts)."""
    return _stage_ms(device, "sl_mesh_fill_stats",
                     ("side_keys_ms", "sort_ms", "boundary_ms", "union_ms", "loops_ms", "caps_ms"))


def quantile(values, q: float) -> float:
    """numpy.quantile(values, q) (linear), the sort on the device."""
    s = torch.sort(values.reshape(-1)).values
    pos = q * (len(s) - 1)
    lo = int(np.floor(pos))
    hi = min(lo + 1, len(s) - 1)
    a, b = (float(x) for x in s[[lo, hi]].cpu().numpy())
    t = pos - lo
    d = b - a
    return b - d * (1.0 - t) if t >= 0.5 else a + d * t


def trim_by_density(vertices, triangles, densities, q: float, *, device=None):
    """remove_vertices_by_mask(densities < quantile(densities, q))."""
    return remove_vertices_by_mask(vertices, triangles, densities < quantile(densities, q), device=device)


def create_from_point_cloud_poisson(points, normals, depth: int = 8, scale: float = 1.1, *, budget_bytes=None,
                                    timings=None, device=None):
    """TriangleMesh.create_from_point_cloud_poisson -> (vertices f64 [V, 3],
    triangles int32 [T, 3], densities f64 [V]) on the device."""
    f = poisson_field(points, normals, depth, scale, budget_bytes=budget_bytes, timings=timings, device=device)
    chi = f.pop("chi")
    st = _Stages(timings, chi.device)
    verts, tris = extract_isosurface(chi, f["iso"], f["origin"], f["h"], device=chi.device)
    del chi
    st.mark("extract")
    dens = vertex_density(f["W"], verts, f["origin"], f["h"], device=verts.device)
    st.mark("density")
    return verts, tris, dens


BPA_MAX_NEIGHBOURS = 1024  # sl_ball_pivot_max_neighbours(): the points within twice the radius of a point


def _normals_for(points, normals, dev):
    P = _f64(points, dev)
    N = torch.as_tensor(normals)
    if N.dim() != 2 or tuple(N.shape) != tuple(P.shape):
        raise ValueError("a normal per point is needed")
    return P, N.to(device=dev, dtype=torch.float64).contiguous()


def _radius(r) -> float:
    r = float(r)
    if not (np.isfinite(r) and r > 0.0):
        raise ValueError("a ball radius must be finite and positive")
    return r


def _bpa_candidates(eng, P, N, radius, cls, capacity):
    n = P.shape[0]
    count = ctypes.c_int64()
    while True:
        tri = torch.empty((max(capacity, 1), 3), dtype=torch.int32, device=eng.device)
        _call(eng, "sl_ball_pivot_candidates", _ptr(P) if n else None, _ptr(N) if n else None, n, radius,
              _ptr(cls), _ptr(tri), capacity, ctypes.byref(count))
        if count.value <= capacity:
            return tri[: count.value]
        capacity = count.value  # the buffer was too small: once more at the exact size


def ball_pivot_candidates(points, normals, radius, vclass=None, *, device=None) -> torch.Tensor:
    """sl_ball_pivot_candidates -> int32 [C, 3] on the device: the triangles of
    the cloud that have an empty ball of ``radius`` on the side of their three
    normals (csrc/slbpa.inl states the test), among the points that are not
    inner (``vclass`` u8 [N]: 0 orphan, 1 border, 2 inner; None: all orphans);
    wound so that the face normal is on the ball's side, in the lexicographic
    order of the sorted triples.  A point with more than BPA_MAX_NEIGHBOURS
    points within twice the radius raises ValueError."""
    eng = _engine(device)
    P, N = _normals_for(points, normals, eng.device)
    radius = _radius(radius)
    cls = None
    if vclass is not None:
        cls = torch.as_tensor(vclass).to(device=eng.device, dtype=torch.uint8).contiguous().reshape(-1)
        if cls.shape[0] != P.shape[0]:
            raise ValueError("a class per point is needed")
    return _bpa_candidates(eng, P, N, radius, cls, 3 * P.shape[0] + 1024)


def ball_pivot_stats(*, device=None) -> dict:
    """Of this thread's last enumeration (sl_ball_pivot_candidates_stats; a
    measurement aid): host milliseconds per stage, the live queries, the candidates and
    the queries that went to the kernel's second tier (a neighbourhood above its first capacity)."""
    v = _stats(device, "sl_ball_pivot_candidates_stats", 7)
    return {"grid_ms": v[0], "enumerate_ms": v[1], "order_ms": v[2], "live": int(v[3]), "candidates": int(v[4]),
            "second_tier": int(v[6])}


def _edge_keys(T, n):
    """int64 [t, 3] -> (the sorted triples, the keys a n + b (a < b) of their three edges)."""
    S = torch.sort(T.to(torch.int64), 1).values
    return S, torch.stack([S[:, 0] * n + S[:, 1], S[:, 1] * n + S[:, 2], S[:, 0] * n + S[:, 2]], 1)


def _count_in(sorted_keys, keys):
    return torch.searchsorted(sorted_keys, keys, right=True) - torch.searchsorted(sorted_keys, keys)


def _bpa_pass(eng, P, N, radius, M, capacity):
    """One pass (rules 1-6 of csrc/slbpa.inl) over the mesh M int32 [t, 3] -> (the appended triangles
    in rank order, the number the per-edge rule dropped).  Everything stays on the device; the host
    reads the candidate count and one pair of counts."""
    n, dev = P.shape[0], eng.device
    cls = None
    if len(M):
        Sm, em = _edge_keys(M, n)
        mk = torch.sort(em.reshape(-1)).values
        once = (_count_in(mk, mk) == 1).to(torch.int32)
        on_border = torch.zeros(n, dtype=torch.int32, device=dev)
        on_border.index_put_((torch.div(mk, n, rounding_mode="floor"),), once, accumulate=True)
        on_border.index_put_((mk % n,), once, accumulate=True)
        cls = torch.zeros(n, dtype=torch.uint8, device=dev)
        cls[M.reshape(-1).to(torch.int64)] = 2
        cls = torch.where(on_border > 0, torch.ones_like(cls), cls)
    else:
        mk = torch.zeros(0, dtype=torch.int64, device=dev)
    C = _bpa_candidates(eng, P, N, radius, cls, capacity)  # rule 1
    c = len(C)
    if c == 0:
        return C, 0
    S, ek = _edge_keys(C, n)
    cm = _count_in(mk, ek)
    keep = (cm < 2).all(1)  # rule 3
    if len(M):
        # rule 2: an edge has at most two triangles in M, so the triple is in one of two slots
        order = torch.argsort(em[:, 0])
        m_ij, m_k = em[order, 0].contiguous(), Sm[order, 2]
        c_ij = ek[:, 0].contiguous()
        lo = torch.searchsorted(m_ij, c_ij)
        for d in (0, 1):
            at = torch.clamp(lo + d, max=len(M) - 1)
            keep &= ~((m_ij[at] == c_ij) & (m_k[at] == S[:, 2]))
        orphans = (cls[S] == 0).all(1)
        keep &= (cm > 0).any(1) | orphans  # rule 4
    # rule 5: entry 3 rank + slot, stably sorted by edge: by edge, then by rank
    big = torch.iinfo(torch.int64).max
    flat = torch.where(keep[:, None], ek, torch.full_like(ek, big)).reshape(-1)
    sk, order = torch.sort(flat, stable=True)
    place = torch.arange(3 * c, device=dev) - torch.searchsorted(sk, sk)
    bad = ((place >= 2 - _count_in(mk, sk)) & (sk != big)).to(torch.int32)
    hits = torch.zeros(c, dtype=torch.int32, device=dev)
    hits.index_put_((torch.div(order, 3, rounding_mode="floor"),), bad, accumulate=True)
    dropped = keep & (hits > 0)
    keep &= ~dropped
    n_keep, n_drop = torch.stack([keep.sum(), dropped.sum()]).tolist()
    first = torch.argsort(keep.to(torch.uint8), descending=True, stable=True)[:n_keep]
    return C[first], n_drop


def create_from_point_cloud_ball_pivoting(points, normals, radii, *, max_passes: int = 8, info: bool = False,
                                          timings=None, device=None):
    """TriangleMesh.create_from_point_cloud_ball_pivoting(pcd, radii) ->
    (vertices f64 [N, 3], triangles int32 [T, 3]) on the device; the vertices
    are the cloud's points.  Open3D's sequential front is restated in an
    order-free form (csrc/slbpa.inl states the rules, tests/bpa_oracle.py is
    their CPU form, which the result equals exactly): a triangle belongs to the
    surface of radius r iff it has an empty r-ball on the side of its three
    vertex normals; per radius, passes append such triangles at non-inner
    vertices -- seeds among orphans, the others along an existing edge -- and a
    per-edge rule keeps every edge at no more than two triangles, until a pass
    appends nothing (or ``max_passes``).  Triangles come in pass order, then in
    the lexicographic order of their sorted triples; two runs give identical
    arrays.  With ``info`` also {"passes" per radius (the last, empty pass
    included), "triangles" appended per pass, "dropped" by the per-edge rule
    per pass, "border_edges", "converged"}; ``timings`` (a dict) receives per
    pass the radius, the milliseconds and ``ball_pivot_stats`` of its enumeration.
    Deviations: the triangle set is not Open3D's, which depends on its visiting
    order.  Inputs that are not in general position (exact lattices with
    co-spherical quads) are decided by rounding: deterministic, but a quad may
    be covered by both diagonals.  A point with more than BPA_MAX_NEIGHBOURS
    points within twice a radius raises ValueError."""
    eng = _engine(device)
    P, N = _normals_for(points, normals, eng.device)
    radii = [_radius(r) for r in radii]
    if not radii:
        raise ValueError("at least one ball radius is needed")
    max_passes = int(max_passes)
    if max_passes < 1:
        raise ValueError("max_passes must be at least 1")
    n = P.shape[0]
    M = torch.zeros((0, 3), dtype=torch.int32, device=eng.device)
    out = {"passes": [], "triangles": [], "dropped": [], "border_edges": 0, "converged": True}
    capacity = 3 * n + 1024
    for r in radii:
        passes, done = 0, False
        while passes < max_passes and not done:
            st = _Stages(None if timings is None else {}, eng.device)
            new, dropped = _bpa_pass(eng, P, N, r, M, capacity)
            passes += 1
            out["triangles"].append(len(new))
            out["dropped"].append(dropped)
            M = torch.cat([M, new])
            done = len(new) == 0
            if timings is not None:
                st.mark("pass")
                timings.setdefault("radius", []).append(r)
                timings.setdefault("ms", []).append(st.timings["pass"])
                for key, v in ball_pivot_stats(device=eng.device).items():  # of the pass's enumeration
                    timings.setdefault(key, []).append(v)
        out["passes"].append(passes)
        out["converged"] = out["converged"] and done
    if not info:
        return P, M
    if len(M):
        mk = torch.sort(_edge_keys(M, n)[1].reshape(-1)).values
        out["border_edges"] = int((_count_in(mk, mk) == 1).sum())
    return P, M, out


def _host(a, dtype):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(np.asarray(a, dtype=dtype)).reshape(-1, 3)


def _mesh_args(vertices, triangles, device):
    eng = _engine(device)
    V = _f64(vertices, eng.device)
    T = _tris(triangles, eng.device)
    return eng, V, T


def compute_triangle_normals(vertices, triangles, *, device=None) -> torch.Tensor:
    """TriangleMesh.compute_triangle_normals -> f64 [T, 3] on the device: (p1 - p0)
    x (p2 - p0) over its length, zero for a zero-area triangle -- the arithmetic
    of the STL writer, bit for bit (csrc/slmeshwrite.inl states it).  An index
    outside 0 .. V - 1 raises IndexError."""
    eng, V, T = _mesh_args(vertices, triangles, device)
    out = torch.empty((max(len(T), 1), 3), dtype=torch.float64, device=eng.device)
    _call(eng, "sl_mesh_triangle_normals", _ptr(V) if len(V) else None, len(V), _ptr(T) if len(T) else None, len(T),
          _ptr(out))
    return out[: len(T)]


def compute_vertex_normals(vertices, triangles, *, device=None) -> torch.Tensor:
    """TriangleMesh.compute_vertex_normals -> f64 [V, 3] on the device: the unit
    normals of a vertex's triangles summed and normalised; (0, 0, 1) for a
    vertex of no triangle or one whose normals cancel.  Deviation: Open3D adds
    in f64 in triangle order; here every triangle adds llrint(n 2^40) to 64-bit
    integer sums, so the result depends on no order and repeats
    (csrc/slmeshwrite.inl; exact against tests/meshwrite_oracle.py).  An index
    outside 0 .. V - 1 raises IndexError."""
    eng, V, T = _mesh_args(vertices, triangles, device)
    out = torch.empty((max(len(V), 1), 3), dtype=torch.float64, device=eng.device)
    _call(eng, "sl_mesh_vertex_normals", _ptr(V) if len(V) else None, len(V), _ptr(T) if len(T) else None, len(T),
          _ptr(out))
    return out[: len(V)]


def mesh_write_stats(*, device=None) -> dict:
    """Host milliseconds of this thread's last device write (sl_mesh_write_stats; a
    measurement aid): waiting for packed chunks to land, inside write(), in all."""
    return _stage_ms(device, "sl_mesh_write_stats", ("wait_ms", "write_ms", "total_ms"))


_STL_REC = np.dtype([("normal", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")])
_PLY_FACE = np.dtype([("n", "u1"), ("v", "<u4", 3)])
_VN_FIX = 2.0 ** 40
_MESH_EXTS = (".stl", ".ply")


def _mesh_ply_header(n_vertices: int, n_triangles: int, colors: bool = False) -> bytes:
    return (f"ply\nformat binary_little_endian 1.0\ncomment Created by Open3D\nelement vertex {n_vertices}\n"
            "property double x\nproperty double y\nproperty double z\n"
            "property double nx\nproperty double ny\nproperty double nz\n"
            + ("property uchar red\nproperty uchar green\nproperty uchar blue\n" if colors else "") +
            f"element face {n_triangles}\nproperty list uchar uint vertex_indices\nend_header\n").encode("ascii")


def _host_triangle_normals(P, T):
    p0, p1, p2 = P[T[:, 0]], P[T[:, 1]], P[T[:, 2]]
    e1, e2 = p1 - p0, p2 - p0
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where((ln == 0.0)[:, None], 0.0, n / ln[:, None])


def _host_vertex_normals(P, T):
    """compute_vertex_normals in NumPy: the same fixed-point sums (int64, wrapping)."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = _host_triangle_normals(P, T) * _VN_FIX
        q = np.rint(np.where(np.abs(t) < 2.0 ** 62, t, 0.0)).astype(np.int64)
    acc = np.zeros((len(P), 3), dtype=np.int64)
    for j in range(3):
        np.add.at(acc, T[:, j], q)
    s = acc.astype(np.float64)
    ln = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    zero = ~s.any(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = s / ln[:, None]
    out[zero] = (0.0, 0.0, 1.0)
    return out


_PLY_COLOR_VERTEX = np.dtype([("pn", "<f8", 6), ("rgb", "u1", 3)])  # 51 bytes, packed


def _write_host(path, ext, vertices, triangles, colors=None):
    P = _host(vertices, np.float64)
    T = _host(triangles, np.int64)
    if len(T) and (T.min() < 0 or T.max() >= len(P)):
        raise IndexError("triangle index out of range")
    if ext == ".ply":
        rec = np.zeros(len(T), dtype=_PLY_FACE)
        rec["n"] = 3
        rec["v"] = T
        pn = np.concatenate([P, _host_vertex_normals(P, T)], 1).astype("<f8")
        if colors is not None:
            vrec = np.zeros(len(P), dtype=_PLY_COLOR_VERTEX)
            vrec["pn"] = pn
            vrec["rgb"] = _host(colors, np.uint8)[:, ::-1]  # BGR storage -> red green blue
            pn = vrec
        with open(path, "wb") as f:
            f.write(_mesh_ply_header(len(P), len(T), colors is not None))
            pn.tofile(f)
            rec.tofile(f)
        return
    p0, p1, p2 = P[T[:, 0]], P[T[:, 1]], P[T[:, 2]]
    rec = np.zeros(len(T), dtype=_STL_REC)
    rec["normal"] = _host_triangle_normals(P, T)
    with np.errstate(over="ignore"):  # beyond float32: +-inf, as the cast says
        rec["v"][:, 0], rec["v"][:, 1], rec["v"][:, 2] = p0, p1, p2
    with open(path, "wb") as f:
        f.write(b"\0" * 80)
        f.write(np.uint32(len(T)).tobytes())
        rec.tofile(f)


def _write_device(path, ext, vertices, triangles, chunk_triangles=0, colors=None):
    """The device writers (csrc/slmeshwrite.inl, the coloured PLY included).  ``path`` None: packed and copied back, no
    file (measurement)."""
    eng, V, T = _mesh_args(vertices, triangles, vertices.device)
    name = "sl_write_mesh_ply_device" if ext == ".ply" else "sl_write_stl_device"
    extra = ()
    if colors is not None and ext == ".ply":
        C = torch.as_tensor(colors).to(device=eng.device, dtype=torch.uint8).contiguous()
        name, extra = "sl_write_mesh_ply_colors_device", (_ptr(C) if len(C) else None,)
    try:
        _call(eng, name, None if path is None else os.fsencode(path), _ptr(V) if len(V) else None, len(V),
              _ptr(T) if len(T) else None, len(T), *extra, int(chunk_triangles))
    except IndexError:
        raise IndexError("triangle index out of range") from None


def write_triangle_mesh(path, vertices, triangles, *, colors=None, chunk_triangles: int = 0) -> None:
    """o3d.io.write_triangle_mesh for ``.stl`` and ``.ply``, after the
    reference's compute_vertex_normals().  ``.stl``: binary STL (80-byte header,
    the count, per triangle the unit normal, three vertices and a zero attribute,
    float32); normals are taken in f64 from the f64 vertices, and a zero-area
    triangle gets a zero normal.  ``.ply``: Open3D's binary little-endian layout
    (unpinned) -- per vertex six doubles, position and ``compute_vertex_normals``;
    per face the byte 3 and three uint32 -- which keeps the shared vertices.
    ``colors`` (BGR u8 [V, 3], as the clouds hold them): the ``.ply`` header gains
    ``property uchar red / green / blue`` after ``nz`` and every vertex record the
    three bytes (51 in all); an ``.stl`` is written as without them, the format
    has no colours.  A colour array without one row per vertex raises ValueError
    before the path is opened.
    Two CUDA tensors on one device are packed on that device and streamed to the
    file through a ring of two pinned chunks of ``chunk_triangles`` triangles (0:
    655 360); anything else (NumPy, CPU tensors) is packed on the host in NumPy.
    Both routes write the same bytes.  An index outside 0 .. V - 1 raises
    IndexError before the path is opened; another extension raises ValueError."""
    ext = os.path.splitext(str(path))[1].lower()
    if ext not in _MESH_EXTS:
        raise ValueError(f"cannot write {path}: only .stl and .ply are supported")
    if colors is not None and tuple(np.shape(colors) if not hasattr(colors, "shape") else colors.shape) != (
            len(vertices), 3):
        raise ValueError("colors must have one row of three per vertex")
    on_device = (isinstance(vertices, torch.Tensor) and isinstance(triangles, torch.Tensor) and vertices.is_cuda
                 and triangles.is_cuda and vertices.device == triangles.device)
    if on_device:
        _write_device(str(path), ext, vertices, triangles, chunk_triangles, colors)
    else:
        _write_host(path, ext, vertices, triangles, colors if ext == ".ply" else None)


def transfer_colors(points, colors, vertices, radius, *, k: int = 8, max_tiers=None, fill=(128, 128, 128),
                    info: bool = False, device=None):
    """The colours of a cloud carried onto mesh vertices (sl_mesh_transfer_colors;
    csrc/slmeshcolor.inl states the definition) -> BGR u8 [V, 3] on the device.
    Tier t searches the open ball of ``radius * 2**t``; a vertex takes, in the
    first tier whose ball holds a cloud point, the colour of a coincident point
    (the lowest index) or else the blend of its up to ``k`` (1..16) nearest by
    (d2, index) with weights d2_first / d2_i.  Tiers run until the radius exceeds
    the diagonal of the joint bounding box, or ``max_tiers`` of them; a vertex
    still unresolved, a non-finite vertex and every vertex of an empty cloud get
    ``fill`` (BGR) and tier 255.  Deviation: Open3D's Poisson colours come from
    its octree's data field (parity unpinned; exact against
    tests/meshcolor_oracle.py).  With ``info``: also the tier u8 [V] and the
    stats dict of ``transfer_colors_stats``."""
    eng = _engine(device)
    P = _f64(points, eng.device)
    Q = _f64(vertices, eng.device)
    C = torch.as_tensor(colors)
    if C.dim() != 2 or tuple(C.shape) != (len(P), 3):
        raise ValueError("colors must have one row of three per point")
    C = C.to(device=eng.device, dtype=torch.uint8).contiguous()
    f = (ctypes.c_uint8 * 3)(*[int(x) for x in fill])
    m = len(Q)
    out = torch.empty((max(m, 1), 3), dtype=torch.uint8, device=eng.device)
    tier = torch.empty(max(m, 1), dtype=torch.uint8, device=eng.device)
    _call(eng, "sl_mesh_transfer_colors", _ptr(P) if len(P) else None, _ptr(C) if len(P) else None, len(P),
          _ptr(Q) if m else None, m, float(radius), int(k), -1 if max_tiers is None else int(max_tiers), f,
          _ptr(out), _ptr(tier))
    if info:
        return out[:m], tier[:m], transfer_colors_stats(device=eng.device)
    return out[:m]


def transfer_colors_stats(*, device=None) -> dict:
    """This thread's last ``transfer_colors`` (sl_mesh_transfer_colors_stats; a measurement aid): tiers run,
    vertices filled, host milliseconds in the grid builds and in the query passes, vertices resolved per tier
    (the first 16), tiers that ran the one-wave-per-query kernel."""
    v = _stats(device, "sl_mesh_transfer_colors_stats", 21)
    tiers = int(v[0])
    return {"tiers": tiers, "filled": int(v[1]), "grid_ms": v[2], "query_ms": v[3],
            "resolved": [int(x) for x in v[4:4 + min(tiers, 16)]], "wave_tiers": int(v[20])}
