"""Inputs that drive sl_segment_plane (csrc/slplane.inl) down the paths that a
wall behind an object never takes, shared by tests/test_plane_oracle.py (which
proves on the CPU, from tests/plane_oracle.py alone, that each input reaches
its path) and tests/test_gpu_plane_paths.py (which compares the library with
the oracle on the same inputs, bit for bit).

``case(name) -> (points, kwargs)``: the cloud and the oracle's keyword
arguments; ``oracle(name)`` is the oracle's cached answer.  The seeds of the
seed-searched cases are recorded where they are used, with the fact that
decided each; the CPU tests assert those facts again.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import plane_oracle as po

PROB = 0.99999999          # segment_plane's default
PROB_LONG = 1.0 - 1e-16    # k = 63 463 at a fitness of 24 / 288 with ransac_n 3


# ------------------------------------------------------------- the scenes ----
def layers_scene(jitter: bool):
    """12 layers of 24 points: x, y ~ U(0, 100), z = 10 l (+ U(-1e-3, 1e-3)
    with ``jitter``), shuffled; default_rng(3), the same draws either way."""
    rng = np.random.default_rng(3)
    n = 12 * 24
    x = rng.uniform(0.0, 100.0, n)
    y = rng.uniform(0.0, 100.0, n)
    z = 10.0 * np.repeat(np.arange(12.0), 24)
    dz = rng.uniform(-1e-3, 1e-3, n)
    perm = rng.permutation(n)
    if jitter:
        z = z + dz
    return np.ascontiguousarray(np.stack([x, y, z], 1)[perm])


def small_wall():
    return po.wall_scene(5001, 0.6)[0]


def wall_diag_scene():
    """small_wall() turned so that the wall's normal (0, 0, 1) becomes
    (1, 1, 1) / sqrt(3); elementwise, so the cloud is the same everywhere."""
    P = small_wall()
    u = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)
    v = np.array([1.0, 1.0, -2.0]) / np.sqrt(6.0)
    w = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
    return np.ascontiguousarray((P[:, 0:1] * u + P[:, 1:2] * v) + P[:, 2:3] * w)


def flat_scene():
    """A 9 x 9 integer lattice on z = 3: every valid hypothesis holds all of it."""
    g = np.stack(np.meshgrid(np.arange(9.0), np.arange(9.0), indexing="ij"), -1).reshape(-1, 2)
    return np.ascontiguousarray(np.concatenate([g, np.full((81, 1), 3.0)], 1))


NONFINITE_SEED = 7
# (draw number whose point is hit, column, value): draws 1, 4 and 6 belong to
# iterations 0, 1 and 2, so the walk builds hypotheses from these points
_NONFINITE_DRAWS = ((1, 0, np.nan), (4, 2, np.inf), (6, 1, -np.inf), (40, 2, np.nan), (70, 0, -np.inf))


def nonfinite_indices():
    n = 5001
    return [po.draw(NONFINITE_SEED, k, n) for k, _, _ in _NONFINITE_DRAWS]


def nonfinite_scene():
    P = small_wall().copy()
    for i, (_, col, val) in zip(nonfinite_indices(), _NONFINITE_DRAWS):
        P[i, col] = val
    return P


def _kw(thr, rn=3, iters=1000, prob=PROB, seed=7):
    return dict(distance_threshold=thr, ransac_n=rn, num_iterations=iters, probability=prob, seed=seed)


# Seeds found by search on the CPU (tests/test_plane_oracle.py asserts each fact):
LAYERS_LATE_SEED = 2     # 375 ties, the winner is tie 332: in the second group of 256
LAYERS_EARLY_SEED = 5    # 400 ties, the winner is tie 87 (layer 1); the second group's best, tie 340, is in layer 10
LAYERS_EXACT_SEED = 2    # 375 ties, all of rmse 0.0; tie 0 in layer 2, 109 ties past 255 in other layers
SCATTER_SEED = 6         # two ties at 35 inliers, the winner is iteration 881
STRICT_SEED = 18         # iteration 0 draws points 58, 619, 373 of the layer z = 1: plane (0, 0, 1, -1)

_CASES = {
    # more than 256 ties on the best count (gap 2)
    "layers_jitter_late": lambda: (layers_scene(True), _kw(1.0, 3, 70_000, PROB_LONG, LAYERS_LATE_SEED)),
    "layers_jitter_early": lambda: (layers_scene(True), _kw(1.0, 3, 70_000, PROB_LONG, LAYERS_EARLY_SEED)),
    "layers_exact": lambda: (layers_scene(False), _kw(1.0, 3, 70_000, PROB_LONG, LAYERS_EXACT_SEED)),
    # batches above 256 hypotheses (gap 1)
    "scatter_1000": lambda: (po.scatter_scene(4099), _kw(2.0, seed=SCATTER_SEED)),
    "wall30": lambda: (po.wall_scene(5001, 0.3)[0], _kw(10.0)),
    # 257 chunks (gap 3)
    "wall_1m": lambda: (po.wall_scene(256 * 4096 + 1, 0.9)[0], _kw(10.0)),
    # the det_x / det_y branches of the final fit (gap 4)
    "wall_x": lambda: (np.ascontiguousarray(small_wall()[:, [2, 0, 1]]), _kw(10.0)),
    "wall_y": lambda: (np.ascontiguousarray(small_wall()[:, [1, 2, 0]]), _kw(10.0)),
    "wall_diag": lambda: (wall_diag_scene(), _kw(10.0)),
    "lattice_x": lambda: (np.ascontiguousarray(po.lattice_scene()[:, [2, 0, 1]]), _kw(0.25, iters=400)),
    "lattice_y": lambda: (np.ascontiguousarray(po.lattice_scene()[:, [1, 2, 0]]), _kw(0.25, iters=400)),
    # the ends of ransac_n (gap 5)
    "rn4": lambda: (small_wall(), _kw(10.0, 4)),
    "rn16": lambda: (small_wall(), _kw(10.0, 16)),
    "rn16_n16": lambda: (po.wall_scene(16, 0.6)[0], _kw(10.0, 16)),
    "rn16_low_fitness_2": lambda: (po.scatter_scene(4099), _kw(2.0, 16, 300)),
    "rn16_low_fitness_20": lambda: (po.scatter_scene(4099), _kw(20.0, 16, 300)),
    # the ends of the walk (gap 6)
    "flat": lambda: (flat_scene(), _kw(0.5, iters=100)),
    "zero_iterations": lambda: (small_wall(), _kw(10.0, iters=0)),
    # a distance exactly equal to the threshold (gap 7)
    "strict_closed": lambda: (po.lattice_scene(), _kw(1.0, iters=1, seed=STRICT_SEED)),
    "strict_open": lambda: (po.lattice_scene(), _kw(float(np.nextafter(1.0, 2.0)), iters=1, seed=STRICT_SEED)),
    # NaN and infinite coordinates (gap 8)
    "nonfinite": lambda: (nonfinite_scene(), _kw(10.0, seed=NONFINITE_SEED)),
    # a last chunk without padding (gap 9)
    "full_chunks_4096": lambda: (po.wall_scene(4096, 0.6)[0], _kw(10.0)),
    "full_chunks_8192": lambda: (po.wall_scene(8192, 0.6)[0], _kw(10.0)),
}
CASES = tuple(_CASES)
BATCH_CASES = ("scatter_1000", "wall30")                                # at batches above 256
TIE_CASES = ("layers_jitter_late", "layers_jitter_early", "layers_exact")  # more than 256 ties


@functools.lru_cache(maxsize=None)
def case(name: str):
    """-> (points f64 [n, 3], the oracle's keyword arguments).  Shared: read only."""
    P, kw = _CASES[name]()
    P.setflags(write=False)
    return P, kw


@functools.lru_cache(maxsize=None)
def oracle(name: str):
    """plane_oracle.segment_plane on the case -> (model, inliers, iterations)."""
    P, kw = case(name)
    model, inl, it = po.segment_plane(P, **kw)
    model.setflags(write=False)
    inl.setflags(write=False)
    return model, inl, it


# ------------------------------------------- facts read off the oracle ----
def _ties(P, thr, rn, seed, result):
    """Every hypothesis of the walk whose count is the final best count ->
    (iteration indices, rmse of each, planes), in iteration order.  A count
    equal to the final best cannot occur before the best first reaches it, so
    these are exactly the hypotheses the walk compares by rmse.  ``result``
    is the oracle's answer on the same arguments."""
    _, inl, it = result
    best = len(inl)
    idx, rmse, planes = [], [], []
    if best == 0:
        return idx, np.zeros(0), planes
    with np.errstate(all="ignore"):
        for i in range(it):
            pl = po.hypothesis(P, seed, i, rn)
            if pl is None:
                continue
            dist = po.distances(P, pl)
            m = dist < thr
            if int(m.sum()) != best:
                continue
            idx.append(i)
            rmse.append(po.ordered_sum(np.where(m, dist, 0.0)) / np.sqrt(float(best)))
            planes.append(pl)
    return idx, np.array(rmse), planes


@functools.lru_cache(maxsize=None)
def ties(name: str):
    """The case's ties -> (iteration indices, rmse, planes), from the cached oracle."""
    P, kw = case(name)
    return _ties(P, kw["distance_threshold"], kw["ransac_n"], kw["seed"], oracle(name))


def tie_report(P, thr, rn, iters, prob, seed):
    """-> the rmse of every hypothesis at the final best count, in iteration order."""
    return tuple(_ties(P, thr, rn, seed, po.segment_plane(P, thr, rn, iters, prob, seed))[1])


def winning_iteration(P, thr, rn, iters, prob, seed):
    """The iteration whose hypothesis the walk keeps: the earliest tie with the
    least rmse (None when no hypothesis ever has an inlier)."""
    idx, rmse, _ = _ties(P, thr, rn, seed, po.segment_plane(P, thr, rn, iters, prob, seed))
    return idx[int(np.argmin(rmse))] if idx else None


def fit_determinants(P, inliers):
    """(det_x, det_y, det_z) of the fit over ``inliers``: the oracle's centroid
    and moments (ordered sums), the oracle's expressions."""
    P = np.asarray(P, dtype=np.float64)
    member = np.zeros(len(P), bool)
    member[np.asarray(inliers)] = True
    m = np.float64(member.sum())
    with np.errstate(all="ignore"):
        c = np.array([po.ordered_sum(np.where(member, P[:, k], 0.0)) / m for k in range(3)])
        r = np.where(member[:, None], P - c, 0.0)
    xx, xy, xz, yy, yz, zz = (np.float64(po.ordered_sum(r[:, a] * r[:, b]))
                              for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)))
    return yy * zz - yz * yz, xx * zz - xz * xz, xx * yy - xy * xy


def fit_branch(P, inliers) -> str:
    """The branch of plane_from_moments the final fit takes: "x", "y" or "z"."""
    det_x, det_y, det_z = fit_determinants(P, inliers)
    if det_x > det_y and det_x > det_z:
        return "x"
    return "y" if det_y > det_z else "z"


def first_valid(P, rn, seed, with_inlier_below=None):
    """The first iteration whose hypothesis is valid (and, with a threshold,
    has an inlier)."""
    i = 0
    with np.errstate(all="ignore"):
        while True:
            pl = po.hypothesis(P, seed, i, rn)
            if pl is not None and (with_inlier_below is None or (po.distances(P, pl) < with_inlier_below).any()):
                return i
            i += 1
