"""tests/cluster_cases.py against the oracle and the grid restatement, on the
CPU: every cloud holds what it was built for (so tests/test_gpu_cluster_paths.py
stands on no unproved assumption), deliberately wrong models of k_ball disagree
with the oracle on the clouds aimed at them (so the cases bite, without a broken
kernel ever running on a GPU), the motif sweep reaches its floors, and the
sequential ClusterDBSCAN loop equals the order-free form on every new cloud."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

from tests import cluster_cases as cc
from tests import cluster_oracle as co

EVERY = list(cc.CASES) + list(cc.SWEEP_SEEDS)
FACE, CORNER = (1, 3, 5, 7), (0, 2, 6, 8)


def _nb(s, i, core_only=False):
    A = s["A"]
    nb = A.indices[A.indptr[i]:A.indptr[i + 1]]
    nb = nb[nb != i]
    return nb[s["counts"][nb] >= s["min_points"]] if core_only else nb


def _clusters(P, eps, mp):
    return co.dbscan_order_free(P, eps, mp)[1]["clusters"]


@pytest.mark.parametrize("name", EVERY)
def test_two_forms_agree(name):
    s = cc.solved(name)
    seq = co.dbscan_sequential(s["P"], s["eps"], s["min_points"], s["A"])
    np.testing.assert_array_equal(seq, s["labels"])
    assert len(s["P"]) <= 8192  # adjacency's every-pair branch


# ---------------------------------------------------------------- the grid ----
def test_grid_restatement_on_a_hand_made_cloud():
    P = np.array([[0.0, 0.0, 0.0], [2.5, 1.5, 3.5], [2.5, 1.5, 2.5], [0.5, 0.5, 0.5], [2.25, 1.75, 3.25]])
    g = cc.grid(P, 1.0)
    assert g.h == 1.0 and g.dims.tolist() == [3, 2, 4] and g.lo.tolist() == [0.0, 0.0, 0.0]
    assert g.key.tolist() == [0, 23, 22, 0, 23]           # (ix 2 + iy) 4 + iz
    assert g.order.tolist() == [0, 3, 2, 1, 4]            # by (key, index)
    assert g.pos.tolist() == [0, 3, 2, 1, 4]
    assert g.run((2, 1, 3), 0, 0) == (2, 5)
    assert g.run((2, 1, 3), -1, 0) == (2, 2) and g.run((2, 1, 3), 1, 0) == (0, 0)  # empty; outside the grid
    assert g.run((1, 1, 1), -1, -1) == (0, 2)
    assert cc.grid(P * 4.0e6, 1.0).h == 14.0              # largest extent / 1e6 above eps
    assert cc.BORDER_ORDER == tuple((0x862075314 >> (4 * e)) & 15 for e in range(9))  # k_ball's constant


@pytest.mark.parametrize("name", [n for n in cc.CASES if not n.startswith(("wave_edge", "radius"))])
def test_anchors_pin_unit_cells_on_the_integers(name):
    s = cc.solved(name)
    g, P = s["grid"], s["P"]
    lo, hi = np.argmin(P.sum(1)), np.argmax(P.sum(1))
    assert g.h == 1.0 and (g.lo == 0.0).all() and (P[lo] == 0.0).all() and (P[hi] == P.max(0)).all()
    np.testing.assert_array_equal(g.ijk, np.floor(P).astype(np.int64))
    rest = np.delete(np.arange(len(P)), [lo, hi])
    for a in (lo, hi):  # at least two cells from everything else: no neighbour cell of anything
        assert np.abs(g.ijk[rest] - g.ijk[a]).max(1).min() >= 2
        assert s["counts"][a] == 1 and s["labels"][a] == -1


# -------------------------------------------------------------------- star ----
@pytest.mark.parametrize("name", cc.STARS)
def test_star(name):
    s = cc.solved(name)
    g, b, mp, labels, counts = s["grid"], s["b"], s["min_points"], s["labels"], s["counts"]
    assert counts[b] == 4 < mp and s["info"]["clusters"] == 3
    near = {k: r[0] for k, r in s["rows"].items()}
    assert sorted(_nb(s, b, core_only=True)) == sorted(near.values())
    col = {k: int(g.column(np.array([b]), np.array([i]))[0]) for k, i in near.items()}
    assert col["own"] == 4 and col["face"] in FACE and col["corner"] in CORNER
    for rank, k in enumerate(s["order"]):  # the row named first is cluster 0
        assert labels[near[k]] == rank and (labels[s["rows"][k]] == rank).all()
    assert labels[b] == 0
    assert cc.border_label_counts(s)[b] == 3
    for k, r in s["rows"].items():  # the far end: a second, uncontested border point
        assert counts[r[-1]] == 4 and cc.border_label_counts(s)[int(r[-1])] == 1 and (counts[r[:-1]] >= mp).all()


def test_each_kind_of_column_holds_label_0_in_two_stars():
    first = [cc.solved(n)["order"][0] for n in cc.STARS]
    assert len(cc.STARS) == 6 and sorted(first) == ["corner"] * 2 + ["face"] * 2 + ["own"] * 2


# -------------------------------------------------------------------- rods ----
@pytest.mark.parametrize("name", ["rods", "rods_mirrored"])
def test_rods(name):
    s = cc.solved(name)
    g, b, mp, labels = s["grid"], s["b"], s["min_points"], s["labels"]
    assert s["counts"][b] == 429 < mp and s["info"] == {"clusters": 2, "core": 1600, "noise": 2}
    a, e = g.run(g.ijk[b], 0, 0)
    assert e - a == 961
    zero, one = ("upper", "lower") if name == "rods" else ("lower", "upper")
    assert (labels[s[zero]] == 0).all() and (labels[s[one]] == 1).all() and (s[zero][0] == 0)
    nb = _nb(s, b, core_only=True)
    assert len(nb) == 428 and (g.column(np.full(len(nb), b), nb) == 4).all()  # all in b's own column
    off = {k: g.pos[nb[np.isin(nb, s[k])]] - a for k in ("upper", "lower")}
    assert off["lower"].max() < 267 <= off["upper"].min() and 267 >= cc.TILE
    assert len(off["lower"]) > 0 and len(off["upper"]) > 0
    if name == "rods":  # every label-1 neighbour before position 267, the first label-0 one in the second tile
        assert off["upper"].min() // cc.TILE == 1
    else:               # label 0 found in the first tile
        assert off["lower"].min() < cc.TILE
    assert labels[b] == 0


# --------------------------------------------------------- dust_then_clump ----
def test_dust_then_clump():
    s = cc.solved("dust_then_clump")
    g, mp, dust, clump = s["grid"], s["min_points"], s["dust"], s["clump"]
    assert s["counts"][dust].max() < mp and (s["counts"][clump] == 230).all() and 230 >= mp
    assert s["info"] == {"clusters": 1, "core": 230, "noise": 302}
    assert len(np.unique(g.ijk[dust][:, :2], axis=0)) == 1 and len(np.unique(g.ijk[clump], axis=0)) == 1
    d = g.ijk[dust[0]][:2] - g.ijk[clump[0]][:2]
    a, e = g.run(g.ijk[clump[0]], int(d[0]), int(d[1]))  # the dust column seen from the clump's cell
    assert e - a == 300 >= cc.TILE and sorted(g.order[a:e]) == sorted(dust)
    assert e <= g.pos[clump].min()                       # all sorted before the clump's
    A = s["A"]
    assert A[clump][:, dust].nnz == 0                    # no dust point within eps of the clump


# ----------------------------------------------------------- two_in_a_cell ----
def test_two_in_a_cell():
    s = cc.solved("two_in_a_cell")
    g = s["grid"]
    assert np.linalg.norm(cc.TWO_A - cc.TWO_B) >= 1.5
    assert s["info"] == {"clusters": 2, "core": 300, "noise": 2}
    assert g.cell_population(s["cell"]) == 300 > cc.TILE
    assert (g.ijk[s["clump_a"]] == s["cell"]).all() and (g.ijk[s["clump_b"]] == s["cell"]).all()
    assert (s["labels"][s["clump_a"]] == 0).all() and (s["labels"][s["clump_b"]] == 1).all()
    assert len(cc.cells_with_two_clusters(s)) == 1
    a, _ = g.run(s["cell"], 0, 0)
    for t in range(0, 300, cc.TILE):  # every tile of the run mixes both trees
        assert set(s["labels"][g.order[a + t:a + min(t + cc.TILE, 300)]]) == {0, 1}
    sizes = np.bincount(s["labels"][s["labels"] >= 0])
    assert sizes.tolist() == [150, 150]  # keep_largest_cluster: equal counts, the lowest label


@pytest.mark.parametrize("name,cut", [("two_in_a_cell_bridged", 2), ("two_in_a_cell_bridged_thin", 1)])
def test_two_in_a_cell_bridged(name, cut):
    """The chain is the only connection.  At spacing 0.4 a chain point also sees the next but one (0.8), so
    no single removal can cut it: there, removing any two consecutive points gives two clusters, and the
    thin chain (0.6) shows the single removal."""
    s = cc.solved(name)
    g, P, chain, mp = s["grid"], s["P"], s["chain"], s["min_points"]
    assert s["info"]["clusters"] == 1 and s["info"]["noise"] == 2 and mp == 3
    step = np.linalg.norm(np.diff(P[chain], axis=0), axis=1)
    np.testing.assert_allclose(step, 0.4 if cut == 2 else 0.6, rtol=0, atol=1e-12)
    assert g.cell_population(s["cell"]) > cc.TILE and (g.ijk[chain] != s["cell"]).any(1).sum() >= 3
    # the chain leaves the shared cell for a cell of higher key, and its points inside the shared cell lie
    # beyond the first tile of the run that the first point outside sees them in
    out = int(np.argmax((g.ijk[chain] != s["cell"]).any(1)))
    assert out >= 1 and g.key[chain[out]] > g.key[chain[0]]
    me = np.full(out, chain[out])
    assert (g.pos[chain[:out]] - g.run_start(me, chain[:out]) >= cc.TILE).all()
    assert _clusters(np.delete(P, chain, axis=0), 1.0, mp) == 2
    for k in range(len(chain) - cut + 1):
        assert _clusters(np.delete(P, chain[k:k + cut], axis=0), 1.0, mp) == 2, k
    where = {int(i): k for k, i in enumerate(chain)}
    for k, i in enumerate(chain):  # no short cut: a chain point's chain neighbours are at most `cut` links away
        assert all(abs(where[int(j)] - k) <= cut for j in _nb(s, i) if int(j) in where)
    for clump, ends in ((s["clump_a"], chain[:cut]), (s["clump_b"], chain[-cut:])):
        assert {int(j) for i in clump for j in _nb(s, i) if int(j) in where} == {int(i) for i in ends}


# --------------------------------------------------------------- tile_edge ----
@pytest.mark.parametrize("L", cc.TILE_EDGE)
def test_tile_edge(L):
    s = cc.solved(f"tile_edge_{L}")
    g, inside, mp = s["grid"], s["inside"], s["min_points"]
    assert len(inside) == L and (g.ijk[inside] == s["cell"]).all() and mp == (3 * L) // 4
    assert g.run(s["cell"], 0, 0) == (1, 1 + L)  # behind the low anchor: the run is exactly L long
    for dx, dy in ((-1, 0), (1, 1), (0, -1)):
        a, e = g.run(s["cell"], dx, dy)
        assert a == e
    core = s["counts"][inside] >= mp
    assert core.any() and (~core).any() and len(np.unique(s["counts"][inside])) > 1
    for t in range(0, L - L % cc.TILE, cc.TILE):  # every whole tile mixes core and non-core candidates
        c = core[g.order[1 + t:1 + t + cc.TILE] - 2]
        assert c.any() and (~c).any()
    half = cc.solved(f"tile_edge_{L}_half")
    np.testing.assert_array_equal(half["P"], s["P"])
    assert half["min_points"] == L // 2 and half["info"]["core"] == L  # why L // 2 is not the mixing setting


# --------------------------------------------------------------- wave_edge ----
@pytest.mark.parametrize("name", [n for n in cc.CASES if n.startswith("wave_edge")])
def test_wave_edge(name):
    s = cc.solved(name)
    g, n = s["grid"], len(s["P"])
    assert n == int(name.split("_")[2]) and n % cc.WAVE in (63, 0, 1)
    assert g.h == 1.0 and g.dims[1] == g.dims[2] == 1
    assert s["info"] == {"clusters": 1, "core": n, "noise": 0}
    x = s["P"][g.order, 0]
    assert (np.diff(np.floor(x)) >= 0).all()  # sorted position runs along the chain, cell by cell
    if name.endswith("in_order"):
        np.testing.assert_array_equal(g.order, np.arange(n))
    else:
        assert (g.order != np.arange(n)).any()
    links = sp.triu(s["A"], 1).tocoo()
    assert links.nnz == n - 1  # connected with n - 1 links: a tree, every link the only connection of its sides
    for edge in range(cc.WAVE, n, cc.WAVE):  # a link crosses every wave boundary
        assert ((g.pos[links.row] < edge) != (g.pos[links.col] < edge)).any()


# ------------------------------------------------------------------- radii ----
def test_degenerate_radii():
    lo, hi = cc.solved("radius_underflow"), cc.solved("radius_overflow")
    assert lo["eps"] > 0.0 and lo["eps"] * lo["eps"] == 0.0 and np.isinf(hi["eps"] * hi["eps"])
    assert (lo["P"][0] == lo["P"][99]).all() and len(np.unique(lo["P"], axis=0)) == 99
    assert (lo["counts"] == 0).all() and lo["info"] == {"clusters": 0, "core": 0, "noise": 100}
    assert (hi["counts"] == 100).all() and hi["info"] == {"clusters": 1, "core": 100, "noise": 0}


# ------------------------------------------------------------ wrong models ----
def model(s, counts=None, keep=None, border="min"):
    """DBSCAN as k_ball computes it, over the adjacency, the sorted positions and the visiting order, with
    parts that can be got wrong: ``counts``; ``keep(g, q, p)``, the links (seen from their later end q) that
    the union pass unites; ``border`` "min", "first" (the first label met in visiting order) or "tile" (only
    the first tile of every run is looked at)."""
    g, mp, n = s["grid"], s["min_points"], len(s["P"])
    core = (s["counts"] if counts is None else counts) >= mp
    A = s["A"].tocoo()
    q, p = A.row.astype(np.int64), A.col.astype(np.int64)
    m = core[q] & core[p] & (g.pos[p] < g.pos[q])
    if keep is not None:
        m &= keep(g, q, p)
    k, comp = connected_components(sp.csr_matrix((np.ones(m.sum(), bool), (q[m], p[m])), shape=(n, n)),
                                   directed=False)
    labels = np.full(n, -1, dtype=np.int32)
    ci = np.nonzero(core)[0]
    smallest = np.full(k, n, dtype=np.int64)
    np.minimum.at(smallest, comp[ci], ci)
    heads = np.sort(smallest[smallest < n])
    labels[ci] = np.searchsorted(heads, smallest[comp[ci]])
    for i in np.nonzero(~core)[0]:
        nb = s["A"].indices[s["A"].indptr[i]:s["A"].indptr[i + 1]].astype(np.int64)
        nb = nb[core[nb]]
        me = np.full(len(nb), i)
        if border == "tile":
            nb = nb[g.pos[nb] - g.run_start(me, nb) < cc.TILE]
        if len(nb) == 0:
            continue
        if border == "first":
            col = np.array([cc.BORDER_ORDER.index(e) for e in g.column(me, nb)])
            labels[i] = labels[nb[np.lexsort((g.pos[nb], col))[0]]]
        else:
            labels[i] = labels[nb].min()
    return labels


def same_wave(g, q, p):
    return g.pos[q] // cc.WAVE == g.pos[p] // cc.WAVE


def first_tile(g, q, p):
    return g.pos[p] - g.run_start(q, p) < cc.TILE


def first_tile_counts(s):
    g = s["grid"]
    A = s["A"].tocoo()
    q, p = A.row.astype(np.int64), A.col.astype(np.int64)
    return np.bincount(q[first_tile(g, q, p)], minlength=len(s["P"])).astype(np.int32)


GRIDDED = [n for n in cc.CASES if not n.startswith("radius")] + list(cc.SWEEP_SEEDS)


@pytest.mark.parametrize("name", GRIDDED)
def test_the_right_model_is_the_oracle(name):
    np.testing.assert_array_equal(model(cc.solved(name)), cc.solved(name)["labels"])


def _differs(name, **wrong):
    s = cc.solved(name)
    return bool((model(s, **wrong) != s["labels"]).any())


def test_wrong_model_first_label_met():
    hit = [n for n in cc.STARS if _differs(n, border="first")]
    assert hit == [n for n in cc.STARS if cc.solved(n)["order"][0] != "own"] and len(hit) == 4
    assert _differs("rods", border="first") and not _differs("rods_mirrored", border="first")
    s = cc.solved("rods")
    assert model(s, border="first")[s["b"]] == 1


def test_wrong_model_border_sees_one_tile():
    s = cc.solved("rods")
    assert model(s, border="tile")[s["b"]] == 1 and _differs("rods", border="tile")
    assert not _differs("rods_mirrored", border="tile")


def test_wrong_model_unions_stay_inside_a_wave():
    for name in [n for n in cc.CASES if n.startswith("wave_edge")]:
        n = len(cc.solved(name)["P"])
        assert _differs(name, keep=same_wave) == (n > cc.WAVE), name
        assert len(np.unique(model(cc.solved(name), keep=same_wave))) == -(-n // cc.WAVE)


def test_wrong_model_unions_see_one_tile():
    """Differs on both bridged clouds: the chain's first points lie in the shared cell behind the 300 clump
    points, so the link from the chain point in the next cell to them is beyond the first tile.  It agrees
    on every tile_edge cloud: a core point beyond the first tile still unites, as a query, with core
    candidates inside it, and those clouds are one blob."""
    for name in ("two_in_a_cell_bridged", "two_in_a_cell_bridged_thin"):
        s = cc.solved(name)
        got = model(s, keep=first_tile)
        assert _differs(name, keep=first_tile) and len(np.unique(got[got >= 0])) == 2
    assert not _differs("two_in_a_cell", keep=first_tile)
    assert [L for L in cc.TILE_EDGE if _differs(f"tile_edge_{L}", keep=first_tile)] == []


def test_wrong_model_counts_see_one_tile():
    for L in cc.TILE_EDGE:
        s = cc.solved(f"tile_edge_{L}")
        assert (first_tile_counts(s) != s["counts"]).any() == (L > cc.TILE), L
    for name in ("rods", "two_in_a_cell", "dust_then_clump"):
        assert (first_tile_counts(cc.solved(name)) != cc.solved(name)["counts"]).any()
    for name in cc.STARS + ["wave_edge_129"]:
        np.testing.assert_array_equal(first_tile_counts(cc.solved(name)), cc.solved(name)["counts"])


# ------------------------------------------------------------------- sweep ----
def test_sweep_reaches_its_floors():
    assert len(cc.SWEEP_SEEDS) == 48 == len(set(cc.SWEEP_SEEDS))
    most = []
    shared = 0
    for seed in cc.SWEEP_SEEDS:
        s = cc.solved(seed)
        assert len(s["P"]) <= 1500 and s["eps"] == 1.0 and s["min_points"] == 5
        assert (s["grid"].dims <= 8).all() and s["grid"].h == 1.0 and (s["grid"].lo == 0.0).all()
        assert len(s["P"]) - len(np.unique(s["P"], axis=0)) >= 3  # the exact duplicates
        most.append(max(cc.border_label_counts(s).values(), default=0))
        shared += len(cc.cells_with_two_clusters(s)) > 0
    most = np.array(most)
    print("border of >= 2 labels:", (most >= 2).sum(), ">= 3:", (most >= 3).sum(), "two clusters in a cell:", shared)
    assert (most >= 2).sum() >= 12
    assert (most >= 3).sum() >= 6
    assert shared >= 8


def test_sweep_is_a_function_of_the_seed():
    np.testing.assert_array_equal(cc.sweep(5)[0], cc.sweep(5)[0])
    assert cc.sweep(5)[0].shape != cc.sweep(6)[0].shape or (cc.sweep(5)[0] != cc.sweep(6)[0]).any()
