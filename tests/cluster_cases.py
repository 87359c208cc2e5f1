"""Clouds that drive k_ball (csrc/slcluster.inl) down the paths that the cases
of tests/cluster_oracle.py never take, shared by tests/test_cluster_cases.py
(which proves on the CPU, from the oracle and the grid restatement below, that
each cloud reaches its path) and tests/test_gpu_cluster_paths.py (which
compares the library with the oracle on the same clouds, exactly).

``grid(P, eps)`` restates build_search_grid / cells / k_cell_neighbours of
csrc/slmerge.hip: the cell edge is max(eps, largest extent / 1e6), the origin
the per-axis minimum, the key (ix ny + iy) nz + iz, and a point's SORTED
POSITION its rank by (key, index) -- a stable sort on the key.  A run is the
sorted positions of the occupied cells (ix + dx, iy + dy, iz - 1 .. iz + 1);
k_ball stages a run in tiles of 256 positions from the run's start, and every
wave owns 64 consecutive positions.

Every constructed cloud but the wave_edge chains (which are their own grid) and
the two degenerate radii has eps = 1 and two lone anchor points, at the minimum
and the maximum corner and no neighbour cell of anything else, so that cells
are unit cubes on the integers.  ``solved(name)`` is the case with the
oracle's answer and the grid, computed once per process.
"""
from __future__ import annotations

import itertools

import numpy as np

from tests import cluster_oracle as co

TILE = 256   # clu::kTile
WAVE = 64    # clu::kW
# k_ball's column order for counts and border labels, as e = 3 (dx + 1) + (dy + 1): the own column, the
# four that share a face with it, the four corner columns; the union pass takes e ascending
BORDER_ORDER = (4, 1, 3, 5, 7, 0, 2, 6, 8)


# ------------------------------------------------------------- the grid ----
class Grid:
    """h, lo, dims, ijk [n, 3], key [n], order (position -> index), pos (index -> position), skey."""

    def __init__(self, P, eps):
        P = np.ascontiguousarray(P, dtype=np.float64)
        self.lo = P.min(0)
        extent = P.max(0) - self.lo
        self.h = max(float(eps), float(extent.max()) / 1.0e6)
        self.dims = np.floor(extent / self.h).astype(np.int64) + 1
        self.ijk = np.floor((P - self.lo) / self.h).astype(np.int64)
        self.key = self.key_of(self.ijk)
        self.order = np.argsort(self.key, kind="stable")
        self.pos = np.empty(len(P), dtype=np.int64)
        self.pos[self.order] = np.arange(len(P))
        self.skey = self.key[self.order]

    def key_of(self, ijk):
        ijk = np.asarray(ijk, dtype=np.int64)
        return (ijk[..., 0] * self.dims[1] + ijk[..., 1]) * self.dims[2] + ijk[..., 2]

    def run(self, cell, dx, dy):
        """[a, b): the sorted positions of the cells (ix + dx, iy + dy, iz - 1 .. iz + 1)."""
        x, y, z = int(cell[0]) + dx, int(cell[1]) + dy, int(cell[2])
        if not (0 <= x < self.dims[0] and 0 <= y < self.dims[1]):
            return 0, 0
        z0, z1 = max(z - 1, 0), min(z + 1, int(self.dims[2]) - 1)
        a = int(np.searchsorted(self.skey, self.key_of(np.array([x, y, z0])), "left"))
        b = int(np.searchsorted(self.skey, self.key_of(np.array([x, y, z1])), "right"))
        return a, b

    def run_start(self, q, p):
        """Per pair (query q, neighbour p): the start of the run of q's cell that holds p."""
        c = self.ijk[q].copy()
        c[:, 0] = self.ijk[p][:, 0]
        c[:, 1] = self.ijk[p][:, 1]
        c[:, 2] = np.maximum(c[:, 2] - 1, 0)
        return np.searchsorted(self.skey, self.key_of(c), "left")

    def column(self, q, p):
        """Per pair: e = 3 (dx + 1) + (dy + 1) of p's column seen from q's cell."""
        d = self.ijk[p] - self.ijk[q]
        return 3 * (d[:, 0] + 1) + (d[:, 1] + 1)

    def cell_population(self, cell):
        k = self.key_of(np.asarray(cell))
        return int(np.searchsorted(self.skey, k, "right") - np.searchsorted(self.skey, k, "left"))


def grid(P, eps):
    return Grid(P, eps)


def _anchors(hi):
    return np.array([[0.0, 0.0, 0.0], list(map(float, hi))])


def _row(start, direction, n=8, spacing=0.3):
    d = np.asarray(direction, dtype=np.float64)
    return np.asarray(start, dtype=np.float64) + spacing * np.arange(n)[:, None] * d


# ----------------------------------------------------------------- star ----
STAR_B = np.array([5.05, 5.05, 5.5])
STAR_DIRS = {"own": np.array([0.0, 0.0, 1.0]), "face": np.array([1.0, 0.0, 0.0]),
             "corner": np.array([-1.0, -1.0, 0.0]) / np.sqrt(2.0)}
STAR_ORDERS = list(itertools.permutations(("own", "face", "corner")))


def star_rows(b, dirs):
    """Three rows of 8 points (spacing 0.3) radiating from b, each near end 0.95 from b."""
    return {k: _row(b + 0.95 * d, d) for k, d in dirs.items()}


def case_star(order):
    """b (4 neighbours: not core at min_points 5) between three rows, one in its own column (+z), one in a
    face column (+x), one in a corner column ((-1, -1, 0) / sqrt 2); the rows' index order is ``order``, so
    the row named first is cluster 0.  Index 0, 1: the anchors; 2: b; then the rows."""
    rows = star_rows(STAR_B, STAR_DIRS)
    P = np.concatenate([_anchors((10, 10, 10)), STAR_B[None]] + [rows[k] for k in order])
    where = {k: np.arange(3 + 8 * i, 11 + 8 * i) for i, k in enumerate(order)}
    return {"P": P, "eps": 1.0, "min_points": 5, "b": 2, "rows": where, "order": order}


# ----------------------------------------------------------------- rods ----
def case_rods(upper_first):
    """Two collinear rods of 800 points along z in one column, z in [2, 3.5] and [4.7, 6.2], and b in the gap
    at z = 4.1 (min_points 480: every rod point is core, b is not).  b's own-column run is the cells iz 3, 4,
    5: the lower rod's top third comes first in it.  ``upper_first``: the upper rod has the lower indices and
    is cluster 0, so b's label-0 neighbours lie beyond the first tile; else the lower rod is cluster 0."""
    t = np.linspace(0.0, 1.5, 800)
    lower = np.stack([np.full(800, 2.5), np.full(800, 2.5), 2.0 + t], 1)
    upper = np.stack([np.full(800, 2.5), np.full(800, 2.5), 4.7 + t], 1)
    b = np.array([[2.5, 2.5, 4.1]])
    first, second = (upper, lower) if upper_first else (lower, upper)
    P = np.concatenate([first, second, b, _anchors((5.5, 5.5, 8.5))])
    return {"P": P, "eps": 1.0, "min_points": 480, "b": 1600,
            "upper": np.arange(800) + (0 if upper_first else 800),
            "lower": np.arange(800) + (800 if upper_first else 0)}


# ------------------------------------------------------ dust_then_clump ----
def case_dust_then_clump():
    """300 dust points in the column (2, 2, 2..4), none of them core at min_points 220, and a clump of 230
    points in the cell (3, 2, 3), whose keys are higher: seen from the clump, the column (dx -1, dy 0) is a
    run of 300 positions without a core candidate, the whole first tile among them."""
    rng = np.random.default_rng(21)
    dust = np.stack([rng.uniform(2.0, 2.5, 300), rng.uniform(2.0, 2.5, 300), rng.uniform(2.0, 5.0, 300)], 1)
    clump = np.array([3.9, 2.25, 3.5]) + rng.uniform(-0.01, 0.01, (230, 3))
    P = np.concatenate([_anchors((6.5, 6.5, 7.5)), dust, clump])
    return {"P": P, "eps": 1.0, "min_points": 220, "dust": np.arange(2, 302), "clump": np.arange(302, 532)}


# ------------------------------------------------------- two_in_a_cell ----
TWO_CELL = np.array([5, 5, 5])
TWO_A = np.array([5.06, 5.06, 5.06])
TWO_B = np.array([5.94, 5.94, 5.94])  # 0.88 sqrt 3 = 1.524 from TWO_A


def two_clumps():
    rng = np.random.default_rng(22)
    both = np.empty((300, 3))
    both[0::2] = TWO_A + rng.uniform(-0.01, 0.01, (150, 3))
    both[1::2] = TWO_B + rng.uniform(-0.01, 0.01, (150, 3))
    return both


def bridge_chain(spacing, straight, radius):
    """A chain from clump A to clump B that leaves the shared cell: ``straight`` steps along +x from A's
    centre, then a circle of ``radius`` in the plane of +x and (0, 1, 1) / sqrt 2, left-hand turn, in chords
    of ``spacing``, up to the first point within 0.8 of B's centre."""
    e1, e2 = np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 1.0]) / np.sqrt(2.0)
    uv = [(spacing * k, 0.0) for k in range(1, straight + 1)]
    centre = (uv[-1][0], radius)
    step = 2.0 * np.arcsin(spacing / (2.0 * radius))
    target = ((TWO_B - TWO_A) @ e1, (TWO_B - TWO_A) @ e2)
    k = 0
    while np.hypot(uv[-1][0] - target[0], uv[-1][1] - target[1]) >= 0.8:
        k += 1
        assert k * step < 2.0 * np.pi
        a = -0.5 * np.pi + k * step
        uv.append((centre[0] + radius * np.cos(a), centre[1] + radius * np.sin(a)))
    uv = np.array(uv)
    return TWO_A + uv[:, :1] * e1 + uv[:, 1:] * e2


def case_two_in_a_cell(bridge=None):
    """Two clumps of 150 points at opposite corners of the cell (5, 5, 5), alternating by index: two
    clusters at min_points 100, and every tile of the cell's run holds core points of both.
    ``bridge`` "wide": min_points 3 and a chain at spacing 0.4 from one clump to the other through the cells
    beyond +x, its indices after the clumps' (its first two points lie in the shared cell, beyond position
    256 of it).  "thin": the same at spacing 0.6, where every chain point has exactly its two chain
    neighbours, so that removing any one of them cuts the chain."""
    parts = [_anchors((10, 10, 10)), two_clumps()]
    c = {"eps": 1.0, "min_points": 100, "clump_a": np.arange(2, 302, 2), "clump_b": np.arange(3, 302, 2),
         "cell": TWO_CELL}
    if bridge is not None:
        chain = bridge_chain(0.4, 5, 1.15) if bridge == "wide" else bridge_chain(0.6, 3, 1.0)
        parts.append(chain)
        c.update(min_points=3, chain=np.arange(302, 302 + len(chain)))
    c["P"] = np.concatenate(parts)
    return c


# ----------------------------------------------------------- tile_edge ----
TILE_EDGE = (255, 256, 257, 511, 512, 513)


def case_tile_edge(L, half=False):
    """L points uniform in the lone cell (3, 3, 3): the cell's run is exactly L long.  min_points is
    3 L // 4, which mixes core and non-core points: the centre of the cell sees all of it, a corner an
    eighth of a unit ball, 52.4 % of it.  (At L // 2, below that share, every point of these clouds is core
    -- the smallest count is 144 of 255 ... 313 of 513 -- and a search of 4000 seeds per size found two
    non-core points once; ``half`` is that all-core setting.)"""
    rng = np.random.default_rng([23, L])
    P = np.concatenate([_anchors((6.5, 6.5, 6.5)), 3.0 + rng.uniform(0.0, 1.0, (L, 3))])
    return {"P": P, "eps": 1.0, "min_points": L // 2 if half else (3 * L) // 4, "cell": np.array([3, 3, 3]),
            "inside": np.arange(2, 2 + L)}


# ----------------------------------------------------------- wave_edge ----
WAVE_EDGE = (63, 64, 65, 127, 128, 129)


def case_wave_edge(n, shuffle=True):
    """A chain of exactly n points along x, spacing 0.6, min_points 2, no anchors: the chain is the grid
    (ny = nz = 1), sorted position runs along it cell by cell, every point is core and every link the only
    connection of its two sides."""
    P = np.stack([0.6 * np.arange(n), np.zeros(n), np.zeros(n)], 1)
    if shuffle:
        P = P[np.random.default_rng([24, n]).permutation(n)]
    return {"P": P, "eps": 1.0, "min_points": 2}


# -------------------------------------------------------------- radii ----
def radius_cloud():
    P = np.random.default_rng(25).uniform(0.0, 3.0, (100, 3))
    P[99] = P[0]  # one exact duplicate pair
    return P


def case_radius_underflow():  # eps eps == 0.0: nobody is a neighbour, not even a point of itself
    return {"P": radius_cloud(), "eps": 1e-170, "min_points": 1}


def case_radius_overflow():   # eps eps == inf: everybody is
    return {"P": radius_cloud(), "eps": 1e160, "min_points": 5}


def _star_name(order):
    return "star_" + "_".join(order)


CASES = {}
for _o in STAR_ORDERS:
    CASES[_star_name(_o)] = (lambda o=_o: case_star(o))
CASES["rods"] = lambda: case_rods(True)
CASES["rods_mirrored"] = lambda: case_rods(False)
CASES["dust_then_clump"] = case_dust_then_clump
CASES["two_in_a_cell"] = case_two_in_a_cell
CASES["two_in_a_cell_bridged"] = lambda: case_two_in_a_cell("wide")
CASES["two_in_a_cell_bridged_thin"] = lambda: case_two_in_a_cell("thin")
for _L in TILE_EDGE:
    CASES[f"tile_edge_{_L}"] = (lambda L=_L: case_tile_edge(L))
    CASES[f"tile_edge_{_L}_half"] = (lambda L=_L: case_tile_edge(L, half=True))
for _n in WAVE_EDGE:
    CASES[f"wave_edge_{_n}"] = (lambda n=_n: case_wave_edge(n))
CASES["wave_edge_129_in_order"] = lambda: case_wave_edge(129, shuffle=False)
CASES["radius_underflow"] = case_radius_underflow
CASES["radius_overflow"] = case_radius_overflow

STARS = [_star_name(o) for o in STAR_ORDERS]


# ---------------------------------------------------------------- sweep ----
SWEEP_EPS, SWEEP_MIN_POINTS, SWEEP_BOX = 1.0, 5, 7.9
SWEEP_SEEDS = tuple(range(48))


def _motif_star(rng):
    return np.concatenate([np.zeros((1, 3))] + list(star_rows(np.zeros(3), STAR_DIRS).values())), False


def _motif_clump_pair(rng):
    na, nb = rng.integers(10, 141, 2)
    a = np.array([0.06, 0.06, 0.06]) + rng.uniform(-0.01, 0.01, (na, 3))
    b = np.array([0.94, 0.94, 0.94]) + rng.uniform(-0.01, 0.01, (nb, 3))
    both = np.concatenate([a, b])
    return both[rng.permutation(len(both))], True  # lives in one unit cell: placed on the integers


def _motif_rod_pair(rng):
    z = 0.2 * np.arange(8)
    rods = np.concatenate([z, z[-1] + 1.9 + z])  # near ends 0.95 either side of the border point
    P = np.zeros((17, 3))
    P[:16, 2] = rods
    P[16, 2] = z[-1] + 0.95
    return P, False


def _motif_chain(rng):
    n = int(rng.integers(6, 14))
    P = np.zeros((n, 3))
    P[:, 0] = 0.45 * np.arange(n)
    return P, False


def _motif_dust(rng):
    n = int(rng.integers(50, 301))
    return rng.uniform(0.0, 1.0, (n, 3)) * rng.uniform(2.0, 6.0, 3), False


MOTIFS = (_motif_star, _motif_clump_pair, _motif_rod_pair, _motif_chain, _motif_dust)


def sweep(seed):
    """2 to 4 motifs at random offsets, axis permutations and reflections in a box of 8 cells per axis,
    three exact duplicates, the two anchors, a random index order -> (P, eps, min_points)."""
    rng = np.random.default_rng([26, seed])
    parts = []
    for kind in rng.integers(0, len(MOTIFS), int(rng.integers(2, 5))):
        pts, in_a_cell = MOTIFS[kind](rng)
        S = np.zeros((3, 3))
        S[np.arange(3), rng.permutation(3)] = rng.choice([-1.0, 1.0], 3)
        if in_a_cell:
            pts = ((pts - 0.5) @ S + 0.5) + rng.integers(0, 8, 3).astype(np.float64)
        else:
            pts = pts @ S
            lo, hi = pts.min(0), pts.max(0)
            pts = pts + (rng.uniform(0.3, (SWEEP_BOX - 0.3) - (hi - lo)) - lo)
        parts.append(pts)
    P = np.concatenate(parts)
    P = np.concatenate([P, P[rng.integers(0, len(P), 3)], _anchors((SWEEP_BOX,) * 3)])
    assert len(P) <= 1500
    return P[rng.permutation(len(P))], SWEEP_EPS, SWEEP_MIN_POINTS


# --------------------------------------------------------------- solved ----
_solved = {}


def _solve(c):
    c["A"] = co.adjacency(c["P"], c["eps"])
    c["labels"], c["info"] = co.dbscan_order_free(c["P"], c["eps"], c["min_points"], c["A"])
    c["counts"] = co.counts_of(c["A"])
    c["grid"] = grid(c["P"], c["eps"])
    for a in (c["P"], c["labels"], c["counts"]):  # shared among the tests: not to be changed
        a.setflags(write=False)
    return c


def solved(name):
    """The case (its own facts, "P", "eps", "min_points") with the oracle's "A", "counts", "labels", "info"
    and the "grid"; ``name`` is a key of CASES or a sweep seed."""
    if name not in _solved:
        if isinstance(name, str):
            c = CASES[name]()
        else:
            P, eps, mp = sweep(name)
            c = {"P": P, "eps": eps, "min_points": mp}
        _solved[name] = _solve(c)
    return _solved[name]


# ---------------------------------------------------- what a cloud holds ----
def border_label_counts(s):
    """Per non-core point with a core neighbour: how many clusters its core neighbours belong to."""
    A, core, labels = s["A"], s["counts"] >= s["min_points"], s["labels"]
    out = {}
    for i in np.nonzero(~core)[0]:
        nb = A.indices[A.indptr[i]:A.indptr[i + 1]]
        nb = nb[core[nb]]
        if len(nb):
            out[int(i)] = len(np.unique(labels[nb]))
    return out


def cells_with_two_clusters(s):
    """The keys of the cells that hold core points of more than one cluster."""
    core = s["counts"] >= s["min_points"]
    pairs = np.unique(np.stack([s["grid"].key[core], s["labels"][core].astype(np.int64)], 1), axis=0)
    keys, n = np.unique(pairs[:, 0], return_counts=True)
    return keys[n > 1]
