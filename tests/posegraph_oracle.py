"""CPU restatement of the loop-closing 360 merge (csrc/slinfo.inl, csrc/
slposegraph.inl, merge.full_registration / merge_360_pose_graph): Open3D's
GetInformationMatrixFromPointClouds, its GlobalOptimizationLevenbergMarquardt
(no line process: every edge certain) and the registration loop of
Old/new360Merge.py:96-137.  Open3D is not in this image, so parity with it is
unpinned; this file is the contract the library is tested against.  Test
infrastructure only.

The information matrix is compared bit for bit.  The optimiser is not: its
``vec6`` / ``mat`` call atan2 / sin / cos, and two libms may differ in the last
place.  Both take the trigonometric functions as a parameter so that a test can
nudge every result by one ulp and measure what that does to the poses.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import merge_oracle as mo

BLOCK = mo.ICP_BLOCK  # source points per partial sum

# ------------------------------------------------------ information matrix ----
# entry k of the upper triangle, row-major -> (a, c)
UPPER = [(a, c) for a in range(6) for c in range(a, 6)]


def g_rows(x, y, z):
    """The rows of G for target points (x, y, z) (arrays): r1 = (0, z, -y, 1, 0,
    0), r2 = (-z, 0, x, 0, 1, 0), r3 = (y, -x, 0, 0, 0, 1)."""
    o, l = np.zeros_like(x), np.ones_like(x)
    return [o, z, -y, l, o, o], [-z, o, x, o, l, o], [y, -x, o, o, o, l]


def information_correspondences(source, target, max_distance, transformation):
    """-> corr int64 [n] (-1: none): the nearest target of every moved source
    point with d2 < max_distance^2, lowest index on ties.  An exactly-identity
    transformation moves nothing."""
    Q = np.array(source, dtype=np.float64).reshape(-1, 3)
    M = np.asarray(transformation, dtype=np.float64).reshape(4, 4)
    if not np.array_equal(M, np.eye(4)):
        Q = mo._transform(Q, M)
    return mo.icp_correspondences(Q, np.asarray(target, dtype=np.float64).reshape(-1, 3), max_distance)[0]


def information_matrix(source, target, max_distance, transformation):
    """-> (6x6 f64, correspondences).  Every correspondence adds G^T G, entry
    (a, c) as (r1[a] r1[c] + r2[a] r2[c]) + r3[a] r3[c]; source points in
    blocks of 64, a left fold inside each block (unmatched points skipped:
    they add +0.0 to sums that start at +0.0), the blocks' partial sums folded
    left to right; mirrored."""
    n = len(source)
    T = np.asarray(target, dtype=np.float64).reshape(-1, 3)
    if n == 0 or len(T) == 0:
        return np.zeros((6, 6)), 0
    corr = information_correspondences(source, T, max_distance, transformation)
    ok = corr >= 0
    j = np.where(ok, corr, 0)
    r1, r2, r3 = g_rows(T[j, 0], T[j, 1], T[j, 2])
    C = np.stack([(r1[a] * r1[c] + r2[a] * r2[c]) + r3[a] * r3[c] for a, c in UPPER], axis=1)
    C[~ok] = 0.0
    nb = (n + BLOCK - 1) // BLOCK
    pad = np.zeros((nb * BLOCK, 21))
    pad[:n] = C
    part = np.cumsum(pad.reshape(nb, BLOCK, 21), axis=1)[:, -1, :]
    out = [0.0] * 21
    for b in range(nb):
        for k in range(21):
            out[k] = out[k] + float(part[b, k])
    G = np.zeros((6, 6))
    for k, (a, c) in enumerate(UPPER):
        G[a, c] = G[c, a] = out[k]
    return G, int(G[3, 3])


def information_matrix_plain(source, target, max_distance, transformation):
    """The plain definition: sum of G.T @ G over a brute-force nearest-neighbour search."""
    S = np.asarray(source, dtype=np.float64)
    T = np.asarray(target, dtype=np.float64)
    M = np.asarray(transformation, dtype=np.float64).reshape(4, 4)
    Q = S @ M[:3, :3].T + M[:3, 3]
    out = np.zeros((6, 6))
    cnt = 0
    for q in Q:
        d2 = ((T - q) ** 2).sum(axis=1)
        k = int(np.argmin(d2))
        if d2[k] < max_distance * max_distance:
            x, y, z = T[k]
            G = np.array([[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1]], dtype=np.float64)
            out += G.T @ G
            cnt += 1
    return out, cnt


# -------------------------------------------------------------- pose graph ----
class Trig:
    """The trigonometric functions vec6 / mat use (libm's by default)."""
    sin = staticmethod(math.sin)
    cos = staticmethod(math.cos)
    atan2 = staticmethod(math.atan2)


def nudged(direction):
    """Trig with every result moved one ulp towards direction * inf."""
    to = math.inf * direction

    class Nudged:
        sin = staticmethod(lambda v: float(np.nextafter(math.sin(v), to)))
        cos = staticmethod(lambda v: float(np.nextafter(math.cos(v), to)))
        atan2 = staticmethod(lambda a, b: float(np.nextafter(math.atan2(a, b), to)))
    return Nudged


def _m(M):
    return [[float(v) for v in row] for row in np.asarray(M, dtype=np.float64).reshape(4, 4)]


def vec6(M, trig=Trig):
    sy = math.sqrt(M[0][0] * M[0][0] + M[1][0] * M[1][0])
    if sy >= 1e-6:
        a, b, g = trig.atan2(M[2][1], M[2][2]), trig.atan2(-M[2][0], sy), trig.atan2(M[1][0], M[0][0])
    else:
        a, b, g = trig.atan2(-M[1][2], M[1][1]), trig.atan2(-M[2][0], sy), 0.0
    return [a, b, g, M[0][3], M[1][3], M[2][3]]


def mat(v, trig=Trig):
    ca, sa, cb, sb = trig.cos(v[0]), trig.sin(v[0]), trig.cos(v[1]), trig.sin(v[1])
    cg, sg = trig.cos(v[2]), trig.sin(v[2])
    Rx = [[1.0, 0.0, 0.0], [0.0, ca, -sa], [0.0, sa, ca]]
    Ry = [[cb, 0.0, sb], [0.0, 1.0, 0.0], [-sb, 0.0, cb]]
    Rz = [[cg, -sg, 0.0], [sg, cg, 0.0], [0.0, 0.0, 1.0]]
    R = mo._mat3(Rz, mo._mat3(Ry, Rx))
    return [R[0] + [v[3]], R[1] + [v[4]], R[2] + [v[5]], [0.0, 0.0, 0.0, 1.0]]


def lin6(M):
    return [(M[2][1] - M[1][2]) / 2.0, (M[0][2] - M[2][0]) / 2.0, (M[1][0] - M[0][1]) / 2.0, M[0][3], M[1][3], M[2][3]]


def _generator(a, sign):
    G = [[0.0] * 4 for _ in range(4)]
    if a < 3:
        i, j = [(2, 1), (0, 2), (1, 0)][a]  # rotation about x, y, z: G[i][j] = 1, G[j][i] = -1
        G[i][j] = sign
        G[j][i] = -sign
    else:
        G[a - 3][3] = sign
    return G


GEN = [(_generator(a, 1.0), _generator(a, -1.0)) for a in range(6)]


def _inv(M):
    return _m(mo.rigid_inverse(M))


def _dot(u, v):
    s = 0.0
    for p, q in zip(u, v):
        s = s + p * q
    return s


def edge_terms(Ts, Tt, X, trig=Trig):
    """-> (e [6], J_s [6][6], J_t [6][6]) of one edge: e = vec6(X^-1 T_t^-1 T_s);
    column a of J_s = lin6(((X^-1 T_t^-1) G_a) T_s), of J_t the same with -G_a."""
    A = mo.mat4(_inv(X), _inv(Tt))
    e = vec6(mo.mat4(A, Ts), trig)
    Js = [[0.0] * 6 for _ in range(6)]
    Jt = [[0.0] * 6 for _ in range(6)]
    for a in range(6):
        cs = lin6(mo.mat4(mo.mat4(A, GEN[a][0]), Ts))
        ct = lin6(mo.mat4(mo.mat4(A, GEN[a][1]), Ts))
        for m in range(6):
            Js[m][a] = cs[m]
            Jt[m][a] = ct[m]
    return e, Js, Jt


def edge_residual(Ts, Tt, X, L, trig=Trig):
    """e^T Lambda e of one edge."""
    A = mo.mat4(_inv(X), _inv(Tt))
    e = vec6(mo.mat4(A, Ts), trig)
    return _dot(e, [_dot(L[m], e) for m in range(6)])


def graph_residual(nodes, edges, trig=Trig):
    r = 0.0
    for s, t, X, L in edges:
        r = r + edge_residual(nodes[s], nodes[t], X, L, trig)
    return r


def linearise(nodes, edges, reference_node, trig=Trig):
    """-> (H [6N][6N], b [6N], residual): H += J^T Lambda J (both diagonal and
    both off-diagonal blocks per edge, edges in list order), b -= J^T Lambda e,
    every sum a left fold from 0.0; then the reference node's rows and columns
    of H zeroed, its diagonal 1, its part of b 0."""
    n6 = 6 * len(nodes)
    H = [[0.0] * n6 for _ in range(n6)]
    b = [0.0] * n6
    r = 0.0
    for s, t, X, L in edges:
        e, Js, Jt = edge_terms(nodes[s], nodes[t], X, trig)
        Le = [_dot(L[m], e) for m in range(6)]
        r = r + _dot(e, Le)
        W = []
        for J in (Js, Jt):  # W = J^T Lambda
            W.append([[_dot([J[m][a] for m in range(6)], [L[m][k] for m in range(6)]) for k in range(6)]
                      for a in range(6)])
        for p, (ip, Wp) in enumerate(((s, W[0]), (t, W[1]))):
            for q, (iq, Jq) in enumerate(((s, Js), (t, Jt))):
                for a in range(6):
                    for c in range(6):
                        H[6 * ip + a][6 * iq + c] = H[6 * ip + a][6 * iq + c] + _dot(Wp[a], [Jq[m][c] for m in range(6)])
            for a in range(6):
                b[6 * ip + a] = b[6 * ip + a] - _dot(Wp[a], e)
    for a in range(6 * reference_node, 6 * reference_node + 6):
        for k in range(n6):
            H[a][k] = 0.0
            H[k][a] = 0.0
        H[a][a] = 1.0
        b[a] = 0.0
    return H, b, r


def ldlt_solve(A, b):
    """x of A x = b by A = L D L^T without pivoting, one fixed loop order."""
    n = len(b)
    L = [[0.0] * n for _ in range(n)]
    d = [0.0] * n
    for j in range(n):
        v = 0.0
        for q in range(j):
            v = v + (L[j][q] * d[q]) * L[j][q]
        d[j] = A[j][j] - v
        for i in range(j + 1, n):
            w = 0.0
            for q in range(j):
                w = w + (L[i][q] * d[q]) * L[j][q]
            L[i][j] = (A[i][j] - w) / d[j] if d[j] != 0.0 else math.nan
    x = list(b)
    for i in range(n):
        v = 0.0
        for q in range(i):
            v = v + L[i][q] * x[q]
        x[i] = x[i] - v
    for i in range(n):
        x[i] = x[i] / d[i] if d[i] != 0.0 else math.nan
    for i in range(n - 1, -1, -1):
        v = 0.0
        for q in range(i + 1, n):
            v = v + L[q][i] * x[q]
        x[i] = x[i] - v
    return x


DEFAULT_CRITERIA = dict(max_iteration=100, min_relative_increment=1e-6, min_relative_residual_increment=1e-6,
                        min_right_term=1e-6, min_residual=1e-6, max_iteration_lm=20)


def global_optimization(nodes, edges, reference_node=0, criteria=None, trig=Trig):
    """Levenberg-Marquardt on the pose graph -> (nodes, info).  nodes: 4x4
    poses; edges: (source_id, target_id, transformation 4x4, information 6x6).
    A step whose increment is not finite counts as rejected."""
    c = dict(DEFAULT_CRITERIA, **(criteria or {}))
    nodes = [_m(T) for T in nodes]
    edges = [(int(s), int(t), _m(X), [[float(v) for v in row] for row in np.asarray(L).reshape(6, 6)])
             for s, t, X, L in edges]
    n6 = 6 * len(nodes)
    H, b, r = linearise(nodes, edges, reference_node, trig)
    r0 = r
    lam = 1e-5 * max(H[k][k] for k in range(n6))
    nu = 2.0
    stop = max(abs(v) for v in b) < c["min_right_term"] or r < c["min_residual"]
    it = 0
    while it < c["max_iteration"] and not stop:
        tries = 0
        while True:
            Hl = [row[:] for row in H]
            for k in range(n6):
                Hl[k][k] = Hl[k][k] + lam
            delta = ldlt_solve(Hl, b)
            finite = all(math.isfinite(v) for v in delta)
            rho = -1.0
            if finite:
                x = [v for T in nodes for v in vec6(T, trig)]
                if math.sqrt(_dot(delta, delta)) < c["min_relative_increment"] * (
                        math.sqrt(_dot(x, x)) + c["min_relative_increment"]):
                    stop = True
                    break
                cand = [mo.mat4(mat(delta[6 * i:6 * i + 6], trig), nodes[i]) for i in range(len(nodes))]
                r_new = graph_residual(cand, edges, trig)
                rho = (r - r_new) / (_dot(delta, [lam * dv + bv for dv, bv in zip(delta, b)]) + 1e-3)
            if rho > 0.0:
                if abs(r - r_new) < c["min_relative_residual_increment"] * r:
                    stop = True
                nodes = cand
                H, b, r = linearise(nodes, edges, reference_node, trig)
                if max(abs(v) for v in b) < c["min_right_term"]:
                    stop = True
                t = 2.0 * rho - 1.0
                lam = lam * max(1.0 / 3.0, 1.0 - (t * t) * t)
                nu = 2.0
            else:
                lam = lam * nu
                nu = 2.0 * nu
            tries += 1
            if rho > 0.0 or tries >= c["max_iteration_lm"] or stop:
                break
        it += 1
        if r < c["min_residual"]:
            stop = True
    return [np.array(T) for T in nodes], {"iterations": it, "initial_residual": r0, "final_residual": r}


# ------------------------------------------------------- registration loop ----
def registration_pairs(n):
    """(source_id, target_id) in Old/new360Merge.py:103-106's order: every
    (i, i + 1) and, when n > 2, the closing pair (0, n - 1)."""
    return [(s, t) for s in range(n) for t in range(s + 1, n) if t == s + 1 or (s == 0 and t == n - 1)]


def full_registration(views, voxel_size, seed_poses, max_iteration=30):
    """full_registration with seed poses (no RANSAC) -> (nodes, edges): ICP on
    the full clouds at 0.4 voxel from inverse(seed[t]) @ seed[s], target
    normals radius 2 voxel / max_nn 30, then the information matrix."""
    views = [np.asarray(v, dtype=np.float64) for v in views]
    normals = [mo.estimate_normals(v, voxel_size * 2, 30) for v in views]
    odometry = np.eye(4)
    nodes, edges = [np.eye(4)], []
    d = voxel_size * 0.4
    for s, t in registration_pairs(len(views)):
        init = np.array(mo.mat4(mo.rigid_inverse(seed_poses[t]), np.asarray(seed_poses[s], dtype=np.float64)))
        T = mo.registration_icp_point_to_plane(views[s], views[t], normals[t], d, init, max_iteration)["transformation"]
        info, _ = information_matrix(views[s], views[t], d, T)
        if t == s + 1:
            odometry = np.array(mo.mat4(T, odometry))
            nodes.append(mo.rigid_inverse(odometry))
        edges.append((s, t, T, info))
    return nodes, edges
