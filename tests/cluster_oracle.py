"""CPU restatement of csrc/slcluster.inl: radius counts, DBSCAN, the radius
outlier filter, the nearest-neighbour distance and keep-largest-cluster, as
Open3D defines them (Open3D is not installed: parity with it is unpinned).

Neighbourhood: j is a neighbour of i iff ((dx dx + dy dy) + dz dz) < eps eps,
in f64, in that order, i itself included.  A KD-tree pre-selects pairs with a
slightly larger radius; the decision is that expression's (NumPy's elementwise
products and sums are not fused).

DBSCAN is carried in two forms:

* ``dbscan_sequential``: PointCloud::ClusterDBSCAN's loop -- indices
  ascending; an unlabelled core point opens the next cluster and expands it
  through its neighbours, then through the neighbours of every core point it
  reaches; a point first labelled noise is re-claimed by the first cluster that
  reaches it.  (Open3D pops the frontier from a hash set; the expansion claims
  exactly the points that are reachable and unclaimed, whatever the order
  inside it, so the frontier here advances a level at a time.)
* ``dbscan_order_free``: core = count >= min_points; clusters = connected
  components of the core points; label = rank of the cluster's smallest core
  index; a border point takes the smallest label among its core neighbours'
  clusters; the rest is noise (-1).

tests/test_cluster_oracle.py compares the two on every case below; the GPU is
checked against the order-free form.
"""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree


def _d2(P, i, j):
    d = P[i] - P[j]
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def adjacency(P, eps):
    """The neighbourhood graph, self loops included -> CSR bool [n, n], column indices ascending."""
    P = np.ascontiguousarray(P, dtype=np.float64)
    n = len(P)
    eps = float(eps)
    r2 = eps * eps
    if n <= 8192:  # small (and possibly dense) clouds: every pair, no pre-selection
        M = np.empty((n, n), dtype=bool)
        for a in range(0, n, 256):
            d0 = P[a:a + 256, None, 0] - P[None, :, 0]
            d1 = P[a:a + 256, None, 1] - P[None, :, 1]
            d2 = P[a:a + 256, None, 2] - P[None, :, 2]
            M[a:a + 256] = (d0 * d0 + d1 * d1) + d2 * d2 < r2
        return sp.csr_matrix(M)
    me = np.arange(n, dtype=np.int64)
    i, j = me[:0], me[:0]
    if n > 1:
        pairs = cKDTree(P).query_pairs(eps * (1.0 + 1e-9), output_type="ndarray")
        keep = _d2(P, pairs[:, 0], pairs[:, 1]) < r2
        i, j = pairs[keep, 0].astype(np.int64), pairs[keep, 1].astype(np.int64)
    self_in = me[_d2(P, me, me) < r2]  # 0 < eps eps unless eps eps underflows
    rows = np.concatenate([i, j, self_in])
    cols = np.concatenate([j, i, self_in])
    A = sp.csr_matrix((np.ones(len(rows), dtype=bool), (rows, cols)), shape=(n, n))
    A.sort_indices()
    return A


def counts_of(A):
    return np.diff(A.indptr).astype(np.int32)


def radius_count(P, radius, cap=0, A=None):
    cnt = counts_of(adjacency(P, radius) if A is None else A)
    return np.minimum(cnt, cap).astype(np.int32) if cap > 0 else cnt


def remove_radius_outlier(P, nb_points, radius, A=None):
    if nb_points < 1 or not radius > 0:
        raise ValueError("Illegal input parameters, number of points and radius must be positive")
    return np.nonzero(radius_count(P, radius, A=A) > nb_points)[0].astype(np.int64)


def dbscan_order_free(P, eps, min_points, A=None):
    """-> (labels int32 [n], info {"clusters", "core", "noise"})."""
    A = adjacency(P, eps) if A is None else A
    n = A.shape[0]
    core = counts_of(A) >= min_points
    labels = np.full(n, -1, dtype=np.int32)
    ci = np.nonzero(core)[0]
    k = 0
    if len(ci):
        k, comp = connected_components(A[ci][:, ci], directed=False)
        smallest = np.full(k, n, dtype=np.int64)
        np.minimum.at(smallest, comp, ci)
        rank = np.empty(k, dtype=np.int32)
        rank[np.argsort(smallest)] = np.arange(k, dtype=np.int32)
        labels[ci] = rank[comp]
        # border: the smallest label among the core neighbours (every row holds its diagonal, so none is empty)
        big = np.iinfo(np.int32).max
        col_label = np.where(core[A.indices], labels[A.indices], big)
        if (np.diff(A.indptr) > 0).all():
            row_min = np.minimum.reduceat(col_label, A.indptr[:-1])
        else:
            row_min = np.array([col_label[a:b].min() if b > a else big for a, b in zip(A.indptr[:-1], A.indptr[1:])])
        border = ~core & (row_min != big)
        labels[border] = row_min[border]
    return labels, {"clusters": int(k), "core": int(core.sum()), "noise": int((labels < 0).sum())}


def dbscan_sequential(P, eps, min_points, A=None):
    """PointCloud::ClusterDBSCAN's loop -> labels int32 [n]."""
    A = adjacency(P, eps) if A is None else A
    n = A.shape[0]
    cnt = counts_of(A)
    labels = np.full(n, -2, dtype=np.int32)
    cluster = 0
    for idx in range(n):
        if labels[idx] != -2:
            continue
        if cnt[idx] < min_points:
            labels[idx] = -1
            continue
        visited = np.zeros(n, dtype=bool)
        visited[idx] = True
        labels[idx] = cluster
        frontier = A.indices[A.indptr[idx]:A.indptr[idx + 1]]
        frontier = frontier[~visited[frontier]]
        while len(frontier):
            visited[frontier] = True
            labels[frontier[labels[frontier] == -1]] = cluster  # noise re-claimed as border
            fresh = frontier[labels[frontier] == -2]
            labels[fresh] = cluster
            grow = fresh[cnt[fresh] >= min_points]
            nxt = np.unique(A[grow].indices) if len(grow) else grow
            frontier = nxt[~visited[nxt]]
        cluster += 1
    return labels


def nearest_neighbor_distance(P):
    """sqrt(d2) of the nearest other point (0 for a duplicate, and for n == 1)."""
    P = np.ascontiguousarray(P, dtype=np.float64)
    n = len(P)
    out = np.zeros(n)
    if n < 2:
        return out
    tree = cKDTree(P)
    guess = tree.query(P, k=2)[0][:, 1]
    cand = tree.query_ball_point(P, guess * (1.0 + 1e-9) + 1e-300)
    for i in range(n):
        c = np.asarray(cand[i], dtype=np.int64)
        c = c[c != i]
        out[i] = np.sqrt(_d2(P, np.full(len(c), i), c).min())
    return out


def keep_largest_cluster(labels):
    """Old/StatisticalOutlierRemoval.py:11-29 -> the kept indices (everything when there is no cluster)."""
    labels = np.asarray(labels)
    if len(labels) == 0:
        return np.arange(0)
    unique_labels, counts = np.unique(labels, return_counts=True)
    valid = unique_labels != -1
    unique_labels, counts = unique_labels[valid], counts[valid]
    if len(unique_labels) == 0:
        return np.arange(len(labels))
    return np.where(labels == unique_labels[counts.argmax()])[0]


# ------------------------------------------------------------------ cases ----
def _blob(rng, n, centre, sigma):
    return rng.normal(size=(n, 3)) * sigma + np.asarray(centre, dtype=np.float64)


def case_single():
    return np.array([[1.0, 2.0, 3.0]]), 1.0, 1


def case_fewer_than_min_points():
    return np.random.default_rng(1).uniform(0, 1, (7, 3)), 5.0, 10


def case_min_points_one():
    return np.random.default_rng(2).uniform(0, 10, (500, 3)), 0.8, 1


def case_identical():
    return np.tile([[0.25, -3.0, 7.5]], (300, 1)), 0.5, 10


def case_one_ball():
    return np.random.default_rng(3).uniform(0, 0.5, (5000, 3)), 2.0, 200


def lattice():
    g = np.stack(np.meshgrid(np.arange(6.0), np.arange(5.0), np.arange(4.0), indexing="ij"), -1).reshape(-1, 3)
    return g[np.random.default_rng(4).permutation(len(g))]


def case_lattice_closed():  # points exactly 1 apart are not neighbours
    return lattice(), 1.0, 2


def case_lattice_open():
    return lattice(), float(np.nextafter(1.0, 2.0)), 2


def bridge_rows(order):
    """Two rows of eight core points (spacing 0.3; eps 1, min_points 4) and a lone bridge point within
    eps of exactly one end of each: it sees 3 points.  -> (P, eps, min_points, bridge index).
    order "a": the bridge has index 0 (visited first: noise, then claimed); "b": the row the sequential
    walk reaches first lies behind the other in x and the bridge sits between the rows' indices."""
    row_a = np.stack([0.3 * np.arange(8), np.zeros(8), np.zeros(8)], 1)         # ends at x = 2.1
    row_b = np.stack([4.0 + 0.3 * np.arange(8), np.zeros(8), np.zeros(8)], 1)   # starts at x = 4.0
    bridge = np.array([[3.05, 0.0, 0.0]])
    if order == "a":
        return np.concatenate([bridge, row_a, row_b]), 1.0, 4, 0
    return np.concatenate([row_b[::-1], bridge, row_a]), 1.0, 4, 8


def case_bridge_a():
    return bridge_rows("a")[:3]


def case_bridge_b():
    return bridge_rows("b")[:3]


def case_helix():
    n, eps = 20000, 1.0
    radius, rise = 20.0, 5.0 / (2 * np.pi)  # 5 eps between turns
    t = np.arange(n) * (0.5 * eps / np.hypot(radius, rise))
    P = np.stack([radius * np.cos(t), radius * np.sin(t), rise * t], 1)
    return P[np.random.default_rng(5).permutation(n)], eps, 3


def dense_cell():
    """A blob of 3000 points inside one grid cell (edge eps = 1: two corner points pin the grid's
    origin at 0), a second one of 2999 at the lower indices, sparse noise around them."""
    rng = np.random.default_rng(6)

    def ball(n, centre):
        v = rng.normal(size=(n, 3))
        v *= (0.2 * rng.uniform(0, 1, (n, 1)) ** (1 / 3)) / np.linalg.norm(v, axis=1, keepdims=True)
        return v + centre
    second = ball(2999, np.array([3.5, 12.5, 7.5]))
    corners = np.array([[0.0, 0.0, 0.0], [20.0, 20.0, 20.0]])
    noise = rng.uniform(0, 20, (500, 3))
    first = ball(3000, np.array([14.5, 4.5, 9.5]))
    return np.concatenate([second, corners, noise, first])


def case_dense_cell():
    return dense_cell(), 1.0, 10


def case_wide_extent():
    rng = np.random.default_rng(7)
    return np.concatenate([_blob(rng, 200, (0, 0, 0), 0.5), _blob(rng, 150, (1e7, 0, 0), 0.5)]), 1.0, 5


def case_blobs_and_noise():
    rng = np.random.default_rng(8)
    centres = rng.uniform(15, 85, (6, 3))
    parts = [_blob(rng, 3000, c, 2.0) for c in centres] + [rng.uniform(0, 100, (2000, 3))]
    P = np.concatenate(parts)
    return P[rng.permutation(len(P))], 1.0, 10


def case_equal_twins():
    """A cluster and its exact translate (coordinates on a 1/64 grid, offset 64): equal counts."""
    a = np.random.default_rng(9).integers(0, 64, (60, 3)) / 64.0
    return np.concatenate([a, a + np.array([64.0, 0.0, 0.0])]), 0.5, 3


def case_duplicates():
    P = np.random.default_rng(10).uniform(0, 10, (1000, 3))
    return np.concatenate([P, P[:50]]), 0.8, 4


CASES = {
    "single": case_single,
    "fewer_than_min_points": case_fewer_than_min_points,
    "min_points_one": case_min_points_one,
    "identical": case_identical,
    "one_ball": case_one_ball,
    "lattice_closed": case_lattice_closed,
    "lattice_open": case_lattice_open,
    "bridge_a": case_bridge_a,
    "bridge_b": case_bridge_b,
    "helix": case_helix,
    "dense_cell": case_dense_cell,
    "wide_extent": case_wide_extent,
    "blobs_and_noise": case_blobs_and_noise,
    "equal_twins": case_equal_twins,
    "duplicates": case_duplicates,
}

_solved = {}


def solved(name):
    """The case and its oracle results, computed once per process: {"P", "eps", "min_points", "A",
    "counts", "labels", "info"}."""
    if name not in _solved:
        P, eps, mp = CASES[name]()
        A = adjacency(P, eps)
        labels, info = dbscan_order_free(P, eps, mp, A)
        counts = counts_of(A)
        for a in (labels, counts):  # shared among the tests: not to be changed
            a.setflags(write=False)
        _solved[name] = {"P": P, "eps": eps, "min_points": mp, "A": A, "counts": counts, "labels": labels,
                         "info": info}
    return _solved[name]
