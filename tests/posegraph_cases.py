"""Deterministic inputs of the loop-closing merge's tests -- TEST INFRASTRUCTURE
shared by tests/test_posegraph_oracle.py (which proves by the oracle alone that
every scenario meets its precondition), tests/test_posegraph_host.py and the
GPU tests, which compare the library with tests/posegraph_oracle.py on the same
scenario."""
import functools
import math

import numpy as np

from oracle import merge_oracle as mo
from tests import posegraph_oracle as po
from tests import registration_cases as rc

# ------------------------------------------------------ information matrix ----
BLOB_SIZES = (1, 63, 64, 65, 129, 1000)
MOTION = np.eye(4)
MOTION[:3, :3] = rc.MOTION_R
MOTION[:3, 3] = rc.MOTION_T
INFO_CASES = tuple(f"blob{n}_{m}" for n in BLOB_SIZES for m in ("identity", "moved")) + (
    "gap", "none", "ties", "anchors_2e4", "anchors_1e7")


def _blob_pair(n, seed=0):
    """The first n points of blob(1000), jittered by 0.3 per axis, and the rigid
    copy of all 1000 (the target): at max_distance 0.5 a part of the source has
    no correspondence."""
    P = rc.blob(1000, seed=seed)
    S = P[:n] + np.random.default_rng(100 + n).normal(size=(n, 3)) * 0.3
    return S, mo._transform(P, MOTION)


def info_case(name):
    """-> (source, target, max_distance, transformation).

    blob<n>_moved: the jittered source, moved onto the target by MOTION.
    blob<n>_identity: the same source moved beforehand, and the identity.
    gap: 209 points; the second block of 64 lies 1000 away from the target (a
      whole block without a correspondence) and the last block is partial.
    none: every source point 1000 away.
    ties: registration_cases.icp_ties: every source midway between two targets.
    anchors_2e4 / anchors_1e7: blob1000_moved with the target anchored
      (with_anchors) at max_distance 1: a sparse cell table; at 1e7 also cells
      wider than max_distance."""
    if name.startswith("blob"):
        n, mode = name[4:].split("_")
        S, T = _blob_pair(int(n))
        return (S, T, 0.5, MOTION) if mode == "moved" else (mo._transform(S, MOTION), T, 0.5, np.eye(4))
    if name == "gap":
        S, T = _blob_pair(209)
        S[64:128] += 1000.0
        return S, T, 0.5, MOTION
    if name == "none":
        S, T = _blob_pair(129)
        return S + 1000.0, T, 0.5, MOTION
    if name == "ties":
        S, T, _ = rc.icp_ties()
        return S, T, 1.0, np.eye(4)
    if name.startswith("anchors_"):
        S, T = _blob_pair(1000)
        return S, rc.with_anchors(T, float(name[8:])), 1.0, MOTION
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def info_oracle(name):
    """The oracle's (matrix, count) of a scenario, once per process.  Read only."""
    return po.information_matrix(*info_case(name))


# -------------------------------------------------------------- pose graph ----
GRAPH_CASES = ("ring4", "drift6", "singular")
ZERO = dict(max_iteration=100, min_relative_increment=0.0, min_relative_residual_increment=0.0,
            min_right_term=0.0, min_residual=0.0)


def _spd(rng):
    B = rng.normal(size=(6, 6))
    return (B @ B.T + 6.0 * np.eye(6)) * np.array([50.0, 50.0, 50.0, 1.0, 1.0, 1.0])[:, None] * np.array(
        [50.0, 50.0, 50.0, 1.0, 1.0, 1.0])[None, :]


def _axis_rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)
    return M


def _ring_edges(truth, rng):
    """Exact edges between neighbours and the closing edge, in the registration loop's order."""
    return [(s, t, np.array(mo.mat4(mo.rigid_inverse(truth[t]), truth[s])), _spd(rng))
            for s, t in po.registration_pairs(len(truth))]


def graph_case(name):
    """-> (initial nodes, edges (s, t, X, Lambda), ground-truth nodes).  Every
    edge is exact for the ground truth, X = inverse(T_t) T_s, and node 0 starts
    at its ground truth (it is the reference node).

    ring4: four poses 90 degrees apart about z, the others off by a small motion.
    drift6: six poses 60 degrees apart; node k starts k degrees off about the
      skew axis (1, 2, 3).
    singular: ring4's shape with node 0, which never moves, at beta = pi/2 -
      5e-8: vec6 of that node takes the branch of the Euler singularity in
      every iteration."""
    rng = np.random.default_rng({"ring4": 41, "drift6": 42, "singular": 43}[name])
    if name == "drift6":
        truth = [np.array(po.mat([0.05 * k, -0.03 * k, math.radians(60.0 * k), 10.0 * math.cos(k), 10.0 * math.sin(k),
                                  0.5 * k])) for k in range(6)]
        init = [np.array(mo.mat4(_axis_rotation((1.0, 2.0, 3.0), math.radians(float(k))), T))
                for k, T in enumerate(truth)]
    else:
        truth = [np.array(po.mat([0.02 * k, 0.1, math.radians(90.0 * k) + 0.3, 5.0 * k, -3.0, 1.0 + k]))
                 for k in range(4)]
        if name == "singular":
            truth[0] = np.array(po.mat([0.4, math.pi / 2.0 - 5e-8, -0.7, 1.0, 2.0, 3.0]))
        init = [truth[0]] + [np.array(mo.mat4(po.mat(list(rng.normal(size=6) * 0.01)), T)) for T in truth[1:]]
    return init, _ring_edges(truth, rng), truth


@functools.lru_cache(maxsize=None)
def graph_oracle(name, zero=False, nudge=0):
    """The oracle's (nodes, info) of a graph, once per process: default or ZERO
    criteria; nudge +-1 moves every trigonometric result one ulp.  Read only."""
    init, edges, _ = graph_case(name)
    trig = po.Trig if nudge == 0 else po.nudged(nudge)
    return po.global_optimization(init, edges, 0, ZERO if zero else None, trig)


# The library's optimiser against the oracle's is not bit for bit: libm's atan2 /
# sin / cos and Python's may differ in the last place.  The tolerance comes from
# the oracle alone: nudge_sensitivity() below, the largest change of any output
# pose entry when every trigonometric result moves one ulp up or down, is
# 1.6e-14 on GRAPH_CASES (tests/test_posegraph_host.py checks the figure); the
# tolerance is 16 times that, the factor covering a rounding pattern that
# differs per iteration and not per call.
POSE_NUDGE = 1.6e-14
POSE_FACTOR = 16.0
POSE_TOL = POSE_FACTOR * POSE_NUDGE


def nudge_sensitivity():
    """The largest change of any output pose entry, over GRAPH_CASES, when every
    trigonometric result of the oracle moves one ulp up or down."""
    worst = 0.0
    for name in GRAPH_CASES:
        plain = np.array(graph_oracle(name)[0])
        for direction in (1, -1):
            worst = max(worst, float(np.abs(np.array(graph_oracle(name, False, direction)[0]) - plain).max()))
    return worst


# ------------------------------------------------------------- merge views ----
VOXEL = 4.0


def merge_views(n_points=1500, n_views=4):
    """-> (views, colours, true poses, seed poses).  View k: its own subsample
    (about 70 %) of blob(n_points), moved by the inverse of pose k (90 degrees
    apart about z, with a translation); the seed poses carry an error of k
    degrees about the skew axis (1, 2, 3)."""
    P = rc.blob(n_points, seed=7)
    rng = np.random.default_rng(70)
    views, colours, poses, seeds = [], [], [], []
    for k in range(n_views):
        pose = np.array(po.mat([0.0, 0.0, math.radians(90.0 * k), 3.0 * k, -2.0 * k, 1.0 * k]))
        keep = np.sort(rng.choice(n_points, int(0.7 * n_points), replace=False))
        views.append(mo._transform(P[keep], mo.rigid_inverse(pose)))
        colours.append(rng.integers(0, 256, size=(len(keep), 3), dtype=np.uint8))
        poses.append(pose)
        seeds.append(np.array(mo.mat4(pose, _axis_rotation((1.0, 2.0, 3.0), math.radians(float(k))))))
    return views, colours, poses, seeds
