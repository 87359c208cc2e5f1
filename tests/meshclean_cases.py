"""Named inputs of the mesh clean-up tests (tests/test_meshclean_oracle.py on the CPU,
tests/test_gpu_meshclean.py on the GPU): the smallest shapes at which the kernels of
csrc/slmeshclean.inl can go wrong."""
from __future__ import annotations

import numpy as np

I32 = np.int32


def _t(rows):
    return np.array(rows, dtype=I32).reshape(-1, 3)


def strip(n, seed):
    """n triangles (i, i+1, i+2) over n + 2 vertices whose numbering is shuffled: one component, deep union
    chains."""
    perm = np.random.default_rng(seed).permutation(n + 2)
    i = np.arange(n)
    return perm[np.stack([i, i + 1, i + 2], 1)].astype(I32), n + 2


def random_triples(n_vertices, n, seed):
    """n random index triples below n_vertices; the first two use its top indices."""
    rng = np.random.default_rng(seed)
    T = rng.integers(0, n_vertices, size=(n, 3))
    T[0] = (n_vertices - 1, n_vertices - 2, 0)
    T[1] = (n_vertices - 2, n_vertices - 1, n_vertices - 1)
    return T.astype(I32), n_vertices


def components_cases():
    """name -> (triangles int32 [T, 3], n_vertices)."""
    c = {}
    c["t0"] = (_t([]), 5)
    c["t1"] = (_t([[0, 1, 2]]), 3)
    c["t2_apart"] = (_t([[0, 1, 2], [3, 4, 5]]), 6)
    c["shared_edge"] = (_t([[0, 1, 2], [2, 1, 3]]), 4)
    c["shared_vertex_only"] = (_t([[0, 1, 2], [2, 3, 4]]), 5)
    c["edge_of_3"] = (_t([[0, 1, 2], [0, 1, 3], [1, 0, 4]]), 5)
    c["edge_of_5"] = (_t([[5, 6, 0], [7, 8, 9], [6, 5, 1], [5, 6, 2], [6, 5, 3], [5, 6, 4]]), 10)
    c["same_twice"] = (_t([[0, 1, 2], [3, 4, 5], [0, 1, 2]]), 6)
    c["opposite_windings"] = (_t([[0, 1, 2], [3, 4, 5], [0, 2, 1]]), 6)
    c["degenerate_aab"] = (_t([[0, 0, 1], [1, 0, 2], [3, 3, 4], [5, 5, 5], [5, 5, 6], [7, 8, 9]]), 10)
    # clusters interleaved in index: A = {0, 3, 5}, B = {1, 4}, C = {2}; B's and C's edges sort before A's
    c["interleaved"] = (_t([[10, 11, 12], [0, 1, 2], [5, 6, 7], [11, 12, 13], [1, 2, 3], [12, 13, 14]]), 15)
    for n in (255, 256, 257, 4095, 4096, 4097):
        c[f"strip_{n}"] = strip(n, n)
    i = np.arange(4097)
    c["isolated_4097"] = (np.stack([3 * i, 3 * i + 1, 3 * i + 2], 1).astype(I32), 3 * 4097)
    for v in (15, 16, 17, 255, 256, 257, 65537):
        c[f"v_{v}"] = random_triples(v, 40, v)
    top = 2 ** 31 - 1
    c["v_2_31_minus_1"] = (_t([[top - 1, top - 2, top - 3], [0, 1, 2], [top - 2, top - 1, 0], [2, 1, top - 1],
                               [top - 4, top - 5, top - 6], [top - 3, 7, top - 1]]), top)
    return c


BAD_INDEX_CASES = {"minus_one": (_t([[0, 1, 2], [0, -1, 2]]), 4), "equal_v": (_t([[0, 1, 4], [0, 1, 2]]), 4),
                   "int_max": (_t([[0, 1, 2], [2 ** 31 - 1, 1, 2]]), 4)}


def area_case(seed=9):
    """Clusters of 63, 64, 65, 129 and 1 members, each a fan about an edge of its own (so its members are all
    adjacent and their areas independent), the clusters' triangles interleaved in index; the thirds' distances
    span 10^-6 .. 10^6; some members have zero area (the third on the edge's line, or (a, a, b)).
    -> (vertices f64, triangles int32, the sizes in label order)."""
    rng = np.random.default_rng(seed)
    sizes = [63, 64, 65, 129, 1]
    verts, tris, owner = [], [], []
    for k, n in enumerate(sizes):
        base = len(verts)
        e0 = np.array([10.0 * k, 0.0, 0.0])
        verts += [e0, e0 + np.array([0.0, 1.0 + 0.37 * k, 0.0])]
        for j in range(n):
            d = 10.0 ** rng.uniform(-6.0, 6.0)
            p = e0 + np.array([d * np.cos(j), 0.5, d * np.sin(j)])
            if n > 1 and j % 17 == 5:
                p = e0 + np.array([0.0, -d, 0.0])            # on the edge's line: zero area
            verts.append(p)
            tri = [base, base + 1, base + 2 + j]
            if n > 1 and j % 23 == 7:
                tri = [base, base, base + 1]                # (a, a, b): its edges {a, a} and {a, b}
            tris.append(tri)
            owner.append(k)
    order = rng.permutation(len(tris))   # interleaved in index
    T = _t(tris)[order]
    first = [int(np.nonzero(np.array(owner)[order] == k)[0][0]) for k in range(len(sizes))]
    label_order = np.argsort(first)
    return np.array(verts, dtype=np.float64), T, [sizes[k] for k in label_order]


MASK_SIZES = (0, 1, 4095, 4096, 4097)
MASK_KINDS = ("none", "all", "alternating", "one")


def mask_case(n, kind):
    """-> (vertices f64 [n + 2, 3], triangles int32 [n, 3], mask u8 [n])."""
    T, nv = strip(n, 1000 + n) if n else (_t([]), 2)
    P = np.random.default_rng(n).normal(size=(nv, 3))
    m = np.zeros(n, dtype=np.uint8)
    if kind == "all":
        m[:] = 1
    elif kind == "alternating":
        m[::2] = 1
    elif kind == "one" and n:
        m[n // 2] = 7
    return P, T, m


def unreferenced_cases():
    """name -> (vertices, triangles)."""
    c = {}
    for n in MASK_SIZES:
        P, T, _ = mask_case(n, "none")
        c[f"all_referenced_{n}"] = (P, T)
        extra = np.random.default_rng(n + 1).normal(size=(len(P) + 3, 3))
        c[f"holes_{n}"] = (extra, (T.astype(np.int64) + (T > len(P) // 2) * 3).astype(I32))
    P = np.random.default_rng(3).normal(size=(9, 3))
    c["none_referenced"] = (P, _t([]))
    c["last_only"] = (P, _t([[8, 8, 8]]))
    c["no_vertices"] = (np.zeros((0, 3)), _t([]))
    return c


def live_case(n):
    """n triangles that all survive the mapping (every vertex of the 17^3 lattice is alone in its voxel and no
    triangle repeats an index), so the triple sort and the compaction after it run on exactly n rows.  The last
    triangle is a rotation of the first: a duplicate whose two copies are n - 1 rows apart, and whose third index
    after the rotation, the lattice's last vertex, is the largest and no other triangle's -- the two are the last
    two rows of the first sort's result.  Every 7th triangle in between is a rotation of the one before it."""
    rng = np.random.default_rng(n)
    lattice = np.array([[i, j, k] for i in range(17) for j in range(17) for k in range(17)], dtype=np.float64)
    nv = len(lattice)
    T = np.stack([rng.permutation(nv - 1)[:3] for _ in range(n)])
    T[7::7] = T[6:-1:7][:, [1, 2, 0]]
    T[0] = (5, 6, nv - 1)
    T[n - 1] = (6, nv - 1, 5)
    return lattice[rng.permutation(nv)], T.astype(I32), 0.5


def simplify_cases():
    """name -> (vertices f64, triangles int32, voxel_size)."""
    c = {}
    # lo = -0.25 at voxel 0.5: vertex 1 at 0.25 is exactly on the face between voxels 0 and 1
    c["on_a_face"] = (np.array([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [0.75, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0],
                                [0.24, 0.0, 0.0]]), _t([[0, 1, 3], [1, 2, 3], [5, 2, 4], [0, 5, 3]]), 0.5)
    rng = np.random.default_rng(11)
    P = rng.uniform(-3.0, -1.0, size=(60, 3))
    P[::3, 0] += 2.5   # both signs
    c["negative_coordinates"] = (P, rng.integers(0, 60, size=(90, 3)).astype(I32), 0.4)
    c["one_voxel"] = (rng.uniform(0.0, 0.1, size=(12, 3)), rng.integers(0, 12, size=(9, 3)).astype(I32), 5.0)
    lattice = np.array([[i, j, k] for i in range(3) for j in range(3) for k in range(3)], dtype=np.float64)
    own = rng.permutation(27)
    # every vertex in a voxel of its own: only the rotation changes; all three rotations, a duplicate of the same
    # orientation (dropped) and of the opposite one (kept); the later duplicate (1, 2, 3) sorts before (5, 6, 7)
    c["own_voxels"] = (lattice[own], _t([[5, 6, 7], [1, 2, 3], [2, 3, 1], [3, 1, 2], [1, 3, 2], [9, 8, 4], [8, 4, 9],
                                         [20, 26, 11], [26, 11, 20], [11, 26, 20]]), 0.5)
    P = np.ascontiguousarray(lattice[::-1])      # vertex 0 is (2, 2, 2): the highest voxel key
    c["vertex_0_highest_key"] = (P, _t([[0, 1, 2], [26, 25, 0], [3, 13, 23], [13, 23, 3]]), 0.5)
    # voxels of 1.0: vertices 6 and 7 are unreferenced and alone in a voxel each, 8 unreferenced beside vertex 0
    c["unreferenced_alone"] = (np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 2.0, 0.0], [2.1, 0.1, 0.0],
                                         [0.0, 0.0, 2.0], [0.1, 2.1, 0.0], [5.0, 5.0, 5.0], [4.0, 0.0, 0.0],
                                         [0.1, 0.1, 0.1]]), _t([[0, 1, 2], [3, 5, 4], [0, 3, 5], [1, 3, 4]]), 1.0)
    for n in (4095, 4096, 4097):
        T, nv = strip(n, 50 + n)
        c[f"strip_{n}"] = (np.random.default_rng(n).uniform(0.0, 8.0, size=(nv, 3)), T, 0.9)
    for n in (4095, 4096, 4097):
        c[f"live_{n}"] = live_case(n)
    c["no_triangles"] = (rng.normal(size=(20, 3)), _t([]), 0.7)
    c["nothing"] = (np.zeros((0, 3)), _t([]), 1.0)
    return c


def two_spheres():
    """The unit sphere of 6000 points plus a 0.3-radius sphere of 1500 points at x = 2.2, with outward
    normals -> (points, normals)."""
    from tests import mesh_oracle as mo
    P1, N1 = mo.sphere(6000, (0.0, 0.0, 0.0), seed=0)
    P2, N2 = mo.sphere(1500, (0.0, 0.0, 0.0), seed=1)
    return np.concatenate([P1, 0.3 * P2 + np.array([2.2, 0.0, 0.0])]), np.concatenate([N1, N2])


_SPHERE = {}


def poisson_sphere(depth=6):
    """The depth-6 Poisson mesh of mesh_oracle's unit sphere -> (vertices, triangles, h); computed once."""
    if depth not in _SPHERE:
        from tests import mesh_oracle as mo
        P, N = mo.sphere(20000, (0.1, -0.2, 0.3))
        r = mo.poisson(P, N, depth)
        _SPHERE[depth] = (r["vertices"], r["triangles"], r["h"])
    return _SPHERE[depth]
