"""Deterministic, small inputs built to reach single branches of the merge
primitives (csrc/slmerge.hip: bounds, radix sort, tile scans, segment heads,
cell pyramid, the three kNN kernels) -- TEST INFRASTRUCTURE shared by
tests/test_merge_cases.py, which proves by the oracle alone that every builder
meets its reach condition, and tests/test_gpu_merge_edges.py, which compares
the GPU with the oracle on the same input."""
import functools

import numpy as np

# csrc/slmerge.hip: threads per workgroup, keys per radix-sort / scan tile,
# bits per radix pass, the frontier of the best-first kNN search
KT = 256
RS_TILE = 4096
RS_BITS = 4
BEST_CAP = 4096
# make_grid: the largest floor(extent / voxel) it accepts per axis
GRID_MAX_E = 2_000_000


def _colors(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 3), dtype=np.uint8)


def key_bits(dims):
    """Bits of the largest linear voxel key of a grid (at least 1)."""
    return max(1, (int(dims[0]) * int(dims[1]) * int(dims[2]) - 1).bit_length())


def radix_passes(dims):
    return -(-key_bits(dims) // RS_BITS)


def oracle_grid(points, voxel_size):
    """What oracle/merge_oracle.voxel_down_sample computes on the way: the
    voxel index of every point and the grid dimensions."""
    P = np.asarray(points, dtype=np.float64)
    mn, mx = P.min(0), P.max(0)
    lo = mn - voxel_size * 0.5
    idx = np.floor((P - lo) / voxel_size).astype(np.int64)
    dims = np.floor((mx - lo) / voxel_size).astype(np.int64) + 1
    return idx, dims, lo


def linear_keys(idx, dims):
    """Linear voxel keys as Python ints (no int64 wrap to hide)."""
    d1, d2 = int(dims[1]), int(dims[2])
    return [(int(a) * d1 + int(b)) * d2 + int(c) for a, b, c in idx]


# ------------------------------------------------------- voxel: pass sweep ----
# One cloud per radix pass count 1..16.  voxel_size 1 and points at integer
# voxel corners + jitter in [0, 0.4), with both corners of the box present, so the grid is
# exactly `dims`.  The key width is 4 p - 1 bits split over the axes by a
# pattern that leaves one or two axes flat for small p (dims - 1 where an axis
# is wide enough, so the keys are not all powers of two); p = 16 is the largest
# grid make_grid admits short of its limit, 2 000 000 voxels on every axis.
PASS_COUNTS = tuple(range(1, 17))
PASS_VOXEL = 1.0


def pass_sweep_dims(p):
    if p == 16:
        return (2_000_000, 2_000_000, 2_000_000)
    b = 4 * p - 1
    if p <= 4:  # one wide axis (b <= 15 bits), which one rotates
        bits = [0, 0, 0]
        bits[p % 3] = b
    elif p <= 9:  # two axes (b <= 35), one flat
        bits = [b // 2, b - b // 2, 0]
        bits = bits[p % 3:] + bits[:p % 3]
    else:  # three axes (b <= 59, each <= 20)
        bits = [b // 3, (b + 1) // 3, (b + 2) // 3]
        bits = bits[p % 3:] + bits[:p % 3]
    assert sum(bits) == b and max(bits) <= 20
    return tuple((1 << e) - (1 if e >= 3 else 0) for e in bits)


@functools.lru_cache(maxsize=None)
def pass_sweep(p):
    """-> (points, colours, voxel_size): 1 025 voxels x 4 points = 4 100 points
    (two ragged radix tiles), the first two voxels the box's corners."""
    dims = np.array(pass_sweep_dims(p), dtype=np.int64)
    rng = np.random.default_rng(1000 + p)
    vox = np.stack([rng.integers(0, d, 1025) for d in dims], axis=1)
    vox[0] = 0
    vox[1] = dims - 1
    P = np.repeat(vox, 4, axis=0).astype(np.float64) + rng.uniform(0.0, 0.4, (4100, 3))
    P[0] = 0.0
    P[4] = (dims - 1).astype(np.float64)
    order = rng.permutation(4100)
    return P[order], _colors(4100, 2000 + p), PASS_VOXEL


# -------------------------------------------------------- voxel: tile edges ----
VOXEL_TILE_N = (2, 3, KT - 1, KT, KT + 1, RS_TILE - 1, RS_TILE, RS_TILE + 1, 2 * RS_TILE, 2 * RS_TILE + 1)


@functools.lru_cache(maxsize=None)
def voxel_tile_edge(n):
    """n points, about four per voxel (n = 2, 3: by hand, one voxel of two and,
    for n = 3, a second voxel of one)."""
    if n == 2:
        return np.array([[0.1, 0.2, 0.3], [0.4, 0.1, 0.2]]), np.array([[1, 2, 3], [2, 4, 250]], np.uint8), 1.0
    if n == 3:
        return (np.array([[5.25, 0.0, -1.0], [0.1, 0.2, 0.3], [0.4, 0.1, 0.2]]),
                np.array([[255, 0, 7], [1, 2, 3], [2, 4, 250]], np.uint8), 1.0)
    rng = np.random.default_rng(3000 + n)
    side = (n / 4.0) ** (1.0 / 3.0)
    return rng.uniform(0.0, side, (n, 3)), _colors(n, 3100 + n), 1.0


# -------------------------------------------------------- voxel: long voxel ----
@functools.lru_cache(maxsize=None)
def long_voxel():
    """10 000 points in one voxel (three radix tiles), magnitudes over eight
    decades: the f64 sums depend on the order of the additions."""
    rng = np.random.default_rng(45)
    n = 10_000
    P = rng.uniform(0.0, 1.0, (n, 3)) * 10.0 ** rng.integers(-8, 0, (n, 3))
    return P, _colors(n, 42), 4.0


@functools.lru_cache(maxsize=None)
def one_point_per_voxel():
    """4 097 points, each alone in its voxel (m == n), in shuffled order."""
    rng = np.random.default_rng(43)
    cells = rng.permutation(17 ** 3)[:RS_TILE + 1]
    vox = np.stack([cells // 289, (cells // 17) % 17, cells % 17], axis=1).astype(np.float64)
    return vox + rng.uniform(0.0, 0.4, vox.shape), _colors(len(vox), 44), 1.0


# ------------------------------------------------------- voxel: byte pairs ----
@functools.lru_cache(maxsize=None)
def byte_pairs():
    """65 536 voxels of two points, coloured (a, b) for every byte pair -- the
    pairs in another order in each channel -- and 256 voxels of 255 points of
    one colour each.  All first points come before all second points, then the
    equal-coloured ones.  -> (points, colours, voxel_size, a, b) with a, b the
    (65 536, 3) colours of the pairs in voxel order."""
    rng = np.random.default_rng(51)
    pair = np.arange(65536)
    idx = np.stack([pair, rng.permutation(65536), rng.permutation(65536)], axis=1)
    a, b = (idx >> 8).astype(np.uint8), (idx & 255).astype(np.uint8)
    # voxel_size 1; pair voxel v at (v >> 8, v & 255, 0), equal-colour voxel c at (c, 0, 1)
    centre = np.stack([pair >> 8, pair & 255, np.zeros_like(pair)], axis=1).astype(np.float64)
    eq = np.repeat(np.arange(256), 255)
    eq_centre = np.stack([eq, np.zeros_like(eq), np.ones_like(eq)], axis=1).astype(np.float64)
    P = np.concatenate([centre, centre, eq_centre])
    P += rng.uniform(0.0, 0.4, P.shape)
    C = np.concatenate([a, b, np.repeat(eq.astype(np.uint8)[:, None], 3, axis=1)])
    return P, C, 1.0, a, b


# ------------------------------------------- voxel: faces, inexact quotients ----
FACE_CASES = ("lattice_vs2", "tenths", "tenths_negative", "offset_1e7")


@functools.lru_cache(maxsize=None)
def faces(name):
    rng = np.random.default_rng(61)
    if name == "lattice_vs2":
        # integers 0..7, voxel 2, origin -1: (p + 1) / 2 is an integer at every
        # odd p, the maximum 7 included
        g = np.arange(8, dtype=np.float64)
        P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        P = np.concatenate([P, P[rng.permutation(512)[:300]]])
        vs = 2.0
    elif name == "tenths":
        # k * 0.1 with voxel 0.1 and the minimum at -0.05 (origin -0.1):
        # quotients one ulp either side of an integer
        P = np.concatenate([rng.integers(0, 200, (3000, 3)) * 0.1, [[-0.05, -0.05, -0.05]]])
        vs = 0.1
    elif name == "tenths_negative":
        P = np.concatenate([rng.integers(-150, 50, (3000, 3)) * 0.1, [[-15.05, -15.05, -15.05]]])
        vs = 0.1
    else:
        P = rng.uniform(0.0, 8.0, (3000, 3)) + np.array([1.0e7, -1.0e7, 1.0e7])
        vs = 0.5
    return P[rng.permutation(len(P))], _colors(len(P), 62), vs


# ------------------------------------------------------------ voxel: limits ----
def limit_cloud(e):
    """A cloud whose x axis has exactly e + 1 voxels of size 1 (make_grid's
    floor(extent / voxel) == e), 64 points at each end."""
    rng = np.random.default_rng(71)
    P = rng.uniform(0.0, 0.4, (128, 3))
    P[64:, 0] += float(e)
    P[0] = 0.0
    P[64] = (float(e), 0.0, 0.0)
    return P, _colors(128, 72), 1.0


# ===================================================== statistical outliers ====
def surface_cloud(n, seed, scale=300.0):
    """A bumpy sphere shell + a slab + sparse outliers (surface-like density)."""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    P = u * (scale * (1 + 0.02 * rng.standard_normal((n, 1))))
    P[: n // 5, 2] = rng.uniform(-1, 1, n // 5) * 2 - scale * 1.2
    m = n // 50
    if m:
        P[n - m:] = rng.uniform(-2 * scale, 2 * scale, (m, 3))
    return P


K_SWEEP = (2, 3, 19, 21, 31)
SMALL_N = tuple((k, n) for k in (20, 7) for n in (1, 2, k - 1, k, k + 1))


@functools.lru_cache(maxsize=None)
def sor_tile_edge(n):
    """A tight cluster with every 16th point (0, 16, ...) far away on a wide
    shell: kept and rejected indices in every run of 256, and, at n = 4097,
    a rejected point alone in the last scan tile."""
    rng = np.random.default_rng(4000 + n)
    P = rng.normal(size=(n, 3))
    far = np.arange(0, n, 16)
    u = rng.normal(size=(len(far), 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    P[far] = u * rng.uniform(1000.0, 2000.0, (len(far), 1))
    return P


# Two tight blobs and ten isolated points.  Blob B ends at the maximum corner
# of the bounds (its last point is the corner itself), so it lies in the
# Morton-last cell of every pyramid level; the first isolated point sits
# closer to B than to anything else.
BLOB_N = 1500
BLOB_A = np.array([100.0, 150.0, 80.0])
BLOB_B_CORNER = np.array([1000.0, 900.0, 800.0])


@functools.lru_cache(maxsize=None)
def blob_scene():
    """-> (points, indices of blob B, indices of the isolated points)."""
    rng = np.random.default_rng(91)
    A = BLOB_A + rng.normal(size=(BLOB_N, 3))
    B = BLOB_B_CORNER - rng.uniform(0.0, 2.0, (BLOB_N, 3))
    B[-1] = BLOB_B_CORNER
    iso = np.array([[940.0, 850.0, 760.0],   # nearest to blob B
                    [0.0, 0.0, 0.0], [500.0, 20.0, 400.0], [30.0, 880.0, 10.0], [990.0, 10.0, 790.0],
                    [20.0, 450.0, 795.0], [600.0, 600.0, 300.0], [300.0, 700.0, 650.0], [850.0, 300.0, 50.0],
                    [450.0, 450.0, 780.0]])
    P = np.concatenate([A, B, iso])
    b_idx = np.arange(BLOB_N, 2 * BLOB_N)
    iso_idx = np.arange(2 * BLOB_N, len(P))
    return P, b_idx, iso_idx


# One query at the centre of an exact sphere shell and a few far points: with
# k = 2 the best-first search holds every shell cell in its frontier.
SHELL_N = 25_000
SHELL_K = 2


@functools.lru_cache(maxsize=None)
def shell_scene(n=SHELL_N):
    """-> (points, queries to check against the oracle: the centre, the far
    points and 512 random shell points)."""
    rng = np.random.default_rng(101)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    far = np.array([[0.0, 0.0, 0.0], [700.0, 650.0, 720.0], [-800.0, 30.0, 7.0], [10.0, -750.0, 400.0]])
    P = np.concatenate([u * 300.0, far])
    q = np.concatenate([np.arange(n, n + len(far)), np.sort(rng.permutation(n)[:512])])
    return P, q


DEGENERATE_CASES = ("plane", "line_x", "line_diagonal", "coincident_but_one", "lattice9", "blobs_far")
FAR_OFFSET = 1.0e9
FAR_SCALE = 1.0e-4


@functools.lru_cache(maxsize=None)
def degenerate(name):
    rng = np.random.default_rng(111)
    if name == "plane":
        return np.c_[rng.uniform(0.0, 50.0, (2000, 2)), np.full(2000, 3.25)]
    if name == "line_x":
        return np.c_[rng.uniform(-40.0, 60.0, 1500), np.full(1500, 7.0), np.full(1500, -2.5)]
    if name == "line_diagonal":
        t = rng.uniform(0.0, 100.0, 1500)
        return np.c_[t, t, t]
    if name == "coincident_but_one":
        return np.concatenate([np.repeat([[1.0, 2.0, 3.0]], 39, axis=0), [[4.0, 6.0, 3.5]]])
    if name == "lattice9":
        g = np.arange(9, dtype=np.float64)
        return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    # the blob scene shrunk to spacings near 1e-3 and moved 1e9 from the origin
    return blob_scene()[0] * FAR_SCALE + FAR_OFFSET


# A collinear cloud: two flat axes take the volume floor, the finest cell is
# small against the length, and the Morton keys of the x axis pass 32 bits.
@functools.lru_cache(maxsize=None)
def collinear():
    rng = np.random.default_rng(121)
    x = rng.uniform(0.0, 1000.0, 4000)
    return np.c_[x, np.full(4000, 5.0), np.full(4000, -3.0)]
