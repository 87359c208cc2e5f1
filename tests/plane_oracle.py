"""CPU restatement of sl_segment_plane (csrc/slplane.inl), in NumPy f64.

Open3D's PointCloud::SegmentPlane as one thread runs it, restated from its
published source.  Open3D is not installed here, so parity with Open3D is
UNPINNED: this file is the reference the GPU is checked against, bit for bit.
Two documented deviations from Open3D: the draw is a seeded splitmix64 that
may repeat a point within a sample (Open3D samples without replacement), and
a run in which no hypothesis ever becomes the best returns the zero plane and
no inliers.

Every operation is an IEEE f64 operation in the order slplane.inl's header
states; NumPy's elementwise ``+ - * /`` and ``sqrt`` are exactly those.  Sums
never go through ``np.sum`` (pairwise): ``ordered_sum`` writes the one
summation order out.
"""
from __future__ import annotations

import math

import numpy as np

CHUNK, LANES, ROWS = 4096, 256, 16
_M64 = (1 << 64) - 1


def draw(seed: int, k: int, n: int) -> int:
    """reg::draw (csrc/slreg.inl): the k-th splitmix64 index below n."""
    z = (seed + (k + 1) * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return ((z >> 32) * n) >> 32


def ordered_sum(v) -> float:
    """The ordered sum of v (non-members already +0.0): padded to a multiple of
    4096; in chunk c lane l adds rows v[4096 c + 256 r + l], r = 0..15, to 0.0
    left to right; the tree a[l] += a[l + s], s = 128 .. 1; the chunk sums are
    added to 0.0 left to right."""
    v = np.asarray(v, dtype=np.float64)
    chunks = (len(v) + CHUNK - 1) // CHUNK
    pad = np.zeros(chunks * CHUNK)
    pad[: len(v)] = v
    a = pad.reshape(chunks, ROWS, LANES)
    acc = np.zeros((chunks, LANES))
    for r in range(ROWS):
        acc = acc + a[:, r, :]
    s = LANES // 2
    while s >= 1:
        acc = acc[:, :s] + acc[:, s:2 * s]
        s //= 2
    total = 0.0
    for c in range(chunks):
        total = total + float(acc[c, 0])
    return total


def _plane_from_moments(c, m):
    xx, xy, xz, yy, yz, zz = (np.float64(t) for t in m)
    det_x = yy * zz - yz * yz
    det_y = xx * zz - xz * xz
    det_z = xx * yy - xy * xy
    if det_x > det_y and det_x > det_z:
        nx, ny, nz = det_x, xz * yz - xy * zz, xy * yz - xz * yy
    elif det_y > det_z:
        nx, ny, nz = xz * yz - xy * zz, det_y, xy * xz - yz * xx
    else:
        nx, ny, nz = xy * yz - xz * yy, xy * xz - yz * xx, det_z
    ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
    if ln == 0.0:
        return None
    nx, ny, nz = nx / ln, ny / ln, nz / ln
    d = -((nx * np.float64(c[0]) + ny * np.float64(c[1])) + nz * np.float64(c[2]))
    return np.array([nx, ny, nz, d], dtype=np.float64)


def fit_plane(P, member=None, sequential=False):
    """GetPlaneFromPoints.  ``member`` (bool [n]): the fit over those points of
    the cloud P with ordered sums; ``sequential``: over the rows of P summed
    0.0 + v0 + v1 + ... (a hypothesis's samples in draw order)."""
    P = np.asarray(P, dtype=np.float64)
    if sequential:
        def total(v):
            t = np.float64(0.0)
            for x in v:
                t = t + x
            return t
        m = len(P)
        sel = P
    else:
        total = ordered_sum
        m = int(member.sum())
        sel = np.where(member[:, None], P, 0.0)  # a non-member adds +0.0
    c = [total(sel[:, k]) / np.float64(m) for k in range(3)]
    r = P - np.array(c)
    if not sequential:
        r = np.where(member[:, None], r, 0.0)
    prods = [r[:, 0] * r[:, 0], r[:, 0] * r[:, 1], r[:, 0] * r[:, 2], r[:, 1] * r[:, 1], r[:, 1] * r[:, 2],
             r[:, 2] * r[:, 2]]
    if not sequential:
        prods = [np.where(member, p, 0.0) for p in prods]
    return _plane_from_moments(c, [total(p) for p in prods])


def hypothesis(P, seed: int, i: int, ransac_n: int):
    """Iteration i's plane, or None for an invalid one."""
    n = len(P)
    idx = [draw(seed, ransac_n * i + k, n) for k in range(ransac_n)]
    if ransac_n == 3:
        p0, p1, p2 = P[idx[0]], P[idx[1]], P[idx[2]]
        e0, e1 = p1 - p0, p2 - p0
        nx = e0[1] * e1[2] - e0[2] * e1[1]
        ny = e0[2] * e1[0] - e0[0] * e1[2]
        nz = e0[0] * e1[1] - e0[1] * e1[0]
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        if ln == 0.0:
            return None
        nx, ny, nz = nx / ln, ny / ln, nz / ln
        return np.array([nx, ny, nz, -((nx * p0[0] + ny * p0[1]) + nz * p0[2])])
    return fit_plane(P[idx], sequential=True)


def distances(P, pl):
    return np.abs(((pl[0] * P[:, 0] + pl[1] * P[:, 1]) + pl[2] * P[:, 2]) + pl[3])


def segment_plane(points, distance_threshold, ransac_n=3, num_iterations=100, probability=0.99999999, seed=0):
    """-> (plane_model [4], inliers int64 ascending, iterations run)."""
    P = np.ascontiguousarray(points, dtype=np.float64)
    n = len(P)
    if not 3 <= ransac_n <= 16 or n < ransac_n or num_iterations < 0 or not 0.0 < probability < 1.0:
        raise ValueError("bad segment_plane arguments")
    thr = float(distance_threshold)
    log_p = math.log(1.0 - probability)
    k = float(num_iterations)
    best_count, best_rmse, best_plane = 0, 0.0, None
    i = 0
    with np.errstate(all="ignore"):
        while i < num_iterations and float(i) <= k:
            pl = hypothesis(P, seed, i, ransac_n)
            i += 1
            if pl is None:
                continue
            dist = distances(P, pl)
            inl = dist < thr
            count = int(inl.sum())
            if count < best_count or count == 0:
                continue  # cannot replace the best: (0, 0) only loses to a count > 0
            err = ordered_sum(np.where(inl, dist, 0.0))
            rmse = err / math.sqrt(float(count))
            if count > best_count or rmse < best_rmse:
                best_count, best_rmse, best_plane = count, rmse, pl
                fitness = float(count) / float(n)
                if fitness < 1.0:
                    den = math.log(1.0 - math.pow(fitness, float(ransac_n)))
                    k = min(log_p / den if den != 0.0 else -math.inf, float(num_iterations))
                else:
                    k = 0.0
        if best_plane is None:
            return np.zeros(4), np.zeros(0, np.int64), i
        inl = distances(P, best_plane) < thr
        model = fit_plane(P, member=inl)
    if model is None:
        model = np.zeros(4)
    return model, np.nonzero(inl)[0].astype(np.int64), i


# ---- the scenes the tests share ----
def wall_scene(n=20000, wall_frac=0.6, rng_seed=1):
    """A wall behind an object: wall_frac of the points on z = 800 + N(0, 3)
    with x, y ~ U(-400, 400), the rest on a sphere shell of radius 120 around
    (0, 0, 500); shuffled.  -> (points f64 [n, 3], is_wall bool [n])."""
    rng = np.random.default_rng(rng_seed)
    nw = int(round(n * wall_frac))
    no = n - nw
    wall = np.stack([rng.uniform(-400, 400, nw), rng.uniform(-400, 400, nw), 800 + rng.normal(0, 3, nw)], 1)
    u = rng.normal(size=(no, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    obj = np.array([0.0, 0.0, 500.0]) + 120.0 * u
    P = np.concatenate([wall, obj])
    lab = np.concatenate([np.ones(nw, bool), np.zeros(no, bool)])
    perm = rng.permutation(n)
    return np.ascontiguousarray(P[perm]), lab[perm]


def scatter_scene(n=4099, rng_seed=2):
    """Uniform points in a 1000^3 cube: no plane, so RANSAC never exits early."""
    return np.random.default_rng(rng_seed).uniform(-500, 500, (n, 3))


def lattice_scene():
    """A 17 x 17 x 3 integer lattice: many hypotheses tie on the inlier count."""
    g = np.stack(np.meshgrid(np.arange(17.0), np.arange(17.0), np.arange(3.0), indexing="ij"), -1).reshape(-1, 3)
    return np.ascontiguousarray(g)
