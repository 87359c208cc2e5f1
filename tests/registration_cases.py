"""Deterministic, small inputs built to reach single branches of the global
registration and ICP code (csrc/slreg.inl, csrc/slmerge.hip) -- TEST
INFRASTRUCTURE shared by tests/test_registration_oracle.py, which proves by
the oracle alone that every scenario reaches its branch, and
tests/test_gpu_registration_paths.py, which compares the GPU with the oracle
on the same scenario."""
import functools
import math
import time

import numpy as np

# sl_ransac_feature_matching's batch of hypotheses, its chunk of validations,
# and the cell count above which the target's cell table is searched, not dense
BATCH = 4096
VAL_CHUNK = 256
DENSE_CELLS = 2 ** 26
# sl_radius_search: candidates a query sorts in LDS (more: the radix select)
NN_CAP = 1024


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def blob(n, seed=0):
    """An asymmetric closed surface (a lumpy ellipsoid) sampled at n points."""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    r = 40.0 * (1.0 + 0.25 * np.sin(3.0 * u[:, 0]) * np.cos(2.0 * u[:, 1]) + 0.15 * u[:, 2] ** 3)
    return u * r[:, None] * np.array([1.0, 0.8, 0.6])


MOTION_R = _rot(0.1, 0.35, -0.05)
MOTION_T = np.array([12.0, 0.0, -5.0])


def contaminated(n, p_in, seed):
    """blob(n) and a rigid copy of it; random 33-D source features; the target's
    features equal the source's for a fraction p_in of the points (the
    inliers) and are fresh random rows for the rest -> (source, target,
    source features, target features)."""
    rng = np.random.default_rng(seed)
    P = blob(n, seed=seed)
    Q = P @ MOTION_R.T + MOTION_T
    FS = rng.normal(size=(n, 33))
    FT = FS.copy()
    out = rng.random(n) >= p_in
    FT[out] = rng.normal(size=(int(out.sum()), 33))
    return P, Q, FS, FT


def with_anchors(points, far, features=None):
    """Two more points at (-far, -far, -far) and (far, far, far): the bounding
    box grows, the work does not.  With features: NaN rows for the anchors
    (they never match) -> (points, features)."""
    far = float(far)
    P = np.concatenate([np.asarray(points, dtype=np.float64), np.full((1, 3), -far), np.full((1, 3), far)])
    if features is None:
        return P
    return P, np.concatenate([np.asarray(features, dtype=np.float64), np.full((2, 33), np.nan)])


def grid_cells(points, max_dist):
    """The cell edge and cell count of the grid the GPU builds over a target
    (make_grid: edge max(max_dist, largest extent / 1e6), floor(extent / edge)
    + 1 cells per axis) -> (edge, count as a Python int)."""
    P = np.asarray(points, dtype=np.float64)
    lo, hi = P.min(axis=0), P.max(axis=0)
    h = max(float(max_dist), float((hi - lo).max()) / 1.0e6)
    count = 1
    for k in range(3):
        count *= int(math.floor((hi[k] - lo[k]) / h)) + 1
    return h, count


# ------------------------------------------------------------------ RANSAC ----
# Every scenario: (source, target, source features, target features) and the
# keyword arguments of the oracle's RANSAC (the GPU's under other names, see
# gpu_kwargs).  Seeds and sizes are chosen so that the oracle meets the
# precondition that tests/test_registration_oracle.py asserts for the name.
REFERENCE = dict(edge_sim=0.9, max_iteration=100000, confidence=0.999)
R3_CAPS = (1, BATCH, BATCH + 1)
RANSAC_CASES = ("r1_p07", "r1_p10", "r2", "r3_1", f"r3_{BATCH}", f"r3_{BATCH + 1}", "r4", "r5", "r6_2e4", "r6_1e7")


def _r4():
    """Five points and their rigid copy with two points displaced by far more
    than max_dist; features equal row for row (five correspondences): most
    draws repeat a correspondence."""
    rng = np.random.default_rng(4)
    P = rng.normal(size=(5, 3)) * 10.0
    Q = P @ MOTION_R.T + MOTION_T
    Q[3] += np.array([30.0, -20.0, 25.0])
    Q[4] += np.array([-25.0, 30.0, 20.0])
    F = rng.normal(size=(5, 33))
    return P, Q, F, F.copy()


def _r5():
    """Every source row's nearest target row is one of eight `hubs' (source
    rows scaled towards the origin; the other target rows lie far out), so at
    most eight of 200 pairs are mutual -- fewer than a tenth: the one-way set
    is used.  One source row is NaN and has no neighbour."""
    rng = np.random.default_rng(5)
    n = 200
    P = blob(n, seed=5)
    Q = P @ MOTION_R.T + MOTION_T
    FS = rng.normal(size=(n, 33))
    FT = rng.normal(size=(n, 33)) * 10.0
    FT[:8] = FS[:8] * 0.2
    FS[50] = np.nan
    return P, Q, FS, FT


def ransac_case(name):
    """-> ((source, target, source features, target features), oracle kwargs).

    r1_p07, r1_p10: one-way correspondences with 7 % / 10 % inliers, the
      reference's settings: many batches of hypotheses, stopped by est_k.
    r2: edge similarity 0.5 and confidence 1: a batch with many chunks of
      validations, run to max_iteration = 5000.
    r3_<cap>: r2's cloud (one-way, edge 0.9: a quick oracle) run to exactly
      cap iterations.
    r4: five correspondences, most draws degenerate.
    r5: the mutual filter falls back to the one-way set.
    r6_2e4, r6_1e7: r1_p10 with the target anchored (with_anchors): a sparse
      cell table; at 1e7 with max_dist 1, cells wider than max_dist."""
    if name in ("r1_p07", "r1_p10"):
        p_in, seed = {"r1_p07": (0.07, 6), "r1_p10": (0.10, 5)}[name]
        return contaminated(400, p_in, 3), dict(max_dist=2.0, seed=seed, mutual_filter=False, **REFERENCE)
    if name == "r2":
        return contaminated(150, 0.3, 3), dict(max_dist=2.0, seed=1, mutual_filter=True, edge_sim=0.5,
                                               max_iteration=5000, confidence=1.0)
    if name.startswith("r3_"):
        return contaminated(150, 0.3, 3), dict(max_dist=2.0, seed=1, mutual_filter=False, edge_sim=0.9,
                                               max_iteration=int(name[3:]), confidence=1.0)
    if name == "r4":
        return _r4(), dict(max_dist=1.0, seed=2, mutual_filter=True, edge_sim=0.9, max_iteration=300, confidence=1.0)
    if name == "r5":
        return _r5(), dict(max_dist=2.0, seed=1, mutual_filter=True, edge_sim=0.5, max_iteration=3000,
                           confidence=0.999)
    if name in ("r6_2e4", "r6_1e7"):
        (P, Q, FS, FT), kw = ransac_case("r1_p10")
        Q, FT = with_anchors(Q, float(name[3:]), FT)
        return (P, Q, FS, FT), dict(kw, max_dist=1.0 if name == "r6_1e7" else kw["max_dist"])
    raise KeyError(name)


def gpu_kwargs(kw):
    """The oracle's keyword arguments as merge.registration_ransac_based_on_
    feature_matching's (mutual_filter, max_correspondence_distance), keywords."""
    return (kw["mutual_filter"], kw["max_dist"]), dict(edge_similarity=kw["edge_sim"],
                                                       max_iteration=kw["max_iteration"],
                                                       confidence=kw["confidence"], seed=kw["seed"])


@functools.lru_cache(maxsize=None)
def ransac_oracle(name):
    """The oracle's run of a scenario, once per process -> (result, trace,
    seconds).  Read only."""
    from oracle import registration_oracle as ro
    inputs, kw = ransac_case(name)
    trace = []
    t0 = time.perf_counter()
    res = ro.ransac_based_on_feature_matching(*inputs, trace=trace, **kw)
    return res, trace, time.perf_counter() - t0


def batch_passes(trace):
    """Validated hypotheses per batch of BATCH iterations of an oracle trace."""
    flags = np.array([f for f, _ in trace])
    return [int(np.count_nonzero(flags[a:a + BATCH] == 2)) for a in range(0, len(flags), BATCH)]


# --------------------------------------------------------------------- ICP ----
def icp_ties():
    """-> (source, target, target normals).  The target: a 24 x 24 lattice in
    x, y (z a function of y in eighths, so neighbours in x share it), shuffled,
    with random unit normals; the source: every target point moved by (0.5,
    0, 0.125) -- exactly midway between two targets, which lie in neighbouring
    cells of edge 1."""
    rng = np.random.default_rng(21)
    g = np.arange(24, dtype=np.float64)
    X, Y = (a.ravel() for a in np.meshgrid(g, g, indexing="ij"))
    T = np.stack([X, Y, np.round(24.0 * np.sin(Y / 5.0)) / 8.0], axis=1)[rng.permutation(len(X))]
    N = rng.normal(size=T.shape)
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    return T + np.array([0.5, 0.0, 0.125]), T, N


# ----------------------------------------------------------- radius search ----
RADIUS = 4.0


def cluster(n, seed=0, radius=RADIUS):
    """n points within radius / 2 of the origin: every point is in range of
    every other (an isolated cluster of n candidates per query)."""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return u * (0.49 * radius * rng.random((n, 1)) ** (1.0 / 3.0))


def identical(n=1500):
    return np.repeat(np.array([[1.5, -2.25, 3.0]]), n, axis=0)


LATTICE_RADIUS = 6.5


def lattice(m=15):
    g = np.arange(m, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def scattered(n, seed=0):
    return np.random.default_rng(seed).uniform(-5.0, 5.0, size=(n, 3))


def radius_case(name):
    """-> (points, radius).  c1024 / c1025: the isolated cluster at and one
    past the LDS sort's capacity; identical: 1500 copies of one point;
    lattice: 15 per side, integer d2 with long runs of ties; n<k>: k
    scattered points; a name ending in _far: the same with anchors at 1e7
    (cells wider than the radius)."""
    if name.endswith("_far"):
        P, radius = radius_case(name[:-4])
        return with_anchors(P, 1e7), radius
    if name in ("c1024", "c1025"):
        return cluster(int(name[1:])), RADIUS
    if name == "identical":
        return identical(), RADIUS
    if name == "lattice":
        return lattice(), LATTICE_RADIUS
    if name[0] == "n":
        return scattered(int(name[1:]), seed=int(name[1:])), RADIUS
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def radius_oracle(name):
    """The oracle's complete neighbour lists (no max_nn cut: the lists for a
    max_nn are their first max_nn entries), once per process.  Read only."""
    from oracle import registration_oracle as ro
    P, radius = radius_case(name)
    return ro.radius_neighbours(P, radius, len(P))


# -------------------------------------------------------------------- FPFH ----
FPFH_RADIUS = 5.0


def fpfh_cloud():
    """About 1200 points with every degenerate ingredient of FPFH, the groups
    60 apart: a 65-point plane patch; 40 copies of one point; 100 points on a
    line with normals along it; a block with zero normals; a dense clump with
    hundreds of points in range of each -> (points, normals)."""
    rng = np.random.default_rng(8)

    def unit(v):
        return v / np.linalg.norm(v, axis=1, keepdims=True)
    patch = np.c_[rng.uniform(-6.0, 6.0, (65, 2)), np.zeros(65)]
    patch_n = np.tile([0.0, 0.0, 1.0], (65, 1))
    dup = np.tile([60.0, 1.0, 2.0], (40, 1))
    dup_n = unit(rng.normal(size=(40, 3)))
    around = dup[0] + rng.normal(size=(30, 3)) * 2.0  # neighbours of the copies
    around_n = unit(rng.normal(size=(30, 3)))
    # (eighths along (1, 2, 2): every difference is an exact multiple of the
    # direction, so its cross product with the normal is exactly zero)
    t = np.sort(rng.choice(np.arange(160), 100, replace=False)) / 8.0
    d = np.array([1.0, 2.0, 2.0])
    line = np.array([0.0, 60.0, 0.0]) + t[:, None] * d
    line_n = np.tile(d / 3.0, (100, 1))
    zero = np.array([0.0, 0.0, 60.0]) + rng.uniform(-4.0, 4.0, (100, 3))
    zero_n = np.zeros((100, 3))
    clump = np.array([60.0, 60.0, 0.0]) + rng.normal(size=(865, 3)) * 2.5
    clump_n = unit(rng.normal(size=(865, 3)))
    return (np.concatenate([patch, dup, around, line, zero, clump]),
            np.concatenate([patch_n, dup_n, around_n, line_n, zero_n, clump_n]))
