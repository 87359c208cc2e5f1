"""tests/posegraph_oracle.py proves itself (CPU only): the information matrix
equals the plain definition, and every scenario of tests/posegraph_cases.py
meets the precondition its name promises, so that a GPU test cannot pass by
missing its branch."""
import math

import numpy as np
import pytest

from tests import posegraph_cases as pc
from tests import posegraph_oracle as po
from tests import registration_cases as rc


def _corr(name):
    S, T, d, M = pc.info_case(name)
    return po.information_correspondences(S, T, d, M)


def test_information_matrix_equals_plain_definition():
    S, T, d, M = pc.info_case("blob1000_moved")
    G, cnt = po.information_matrix(S[:300], T, d, M)
    Gp, cntp = po.information_matrix_plain(S[:300], T, d, M)
    assert cnt == cntp and 0 < cnt < 300
    assert np.abs(G - Gp).max() <= 1e-9 * np.abs(Gp).max()


@pytest.mark.parametrize("name", pc.INFO_CASES)
def test_count_on_the_translation_diagonal_and_symmetry(name):
    G, cnt = pc.info_oracle(name)
    assert G[3, 3] == G[4, 4] == G[5, 5] == cnt == int(np.count_nonzero(_corr(name) >= 0))
    assert np.array_equal(G, G.T)


@pytest.mark.parametrize("n", pc.BLOB_SIZES)
def test_blob_cases_match_partly_and_agree_between_identity_and_moved(n):
    """Moving beforehand (identity) or in the call (moved) is the same arithmetic; from 63 points on a
    part of the source, not all of it, has a correspondence, in a dense cell table."""
    a, b = pc.info_oracle(f"blob{n}_identity"), pc.info_oracle(f"blob{n}_moved")
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    if n >= 63:
        assert 0 < a[1] < n
    S, T, d, _ = pc.info_case(f"blob{n}_moved")
    assert rc.grid_cells(T, d)[1] <= rc.DENSE_CELLS


def test_gap_has_an_empty_block_and_a_partial_last_block():
    corr = _corr("gap")
    assert len(corr) % po.BLOCK != 0 and len(corr) > 3 * po.BLOCK
    assert (corr[64:128] < 0).all()
    assert (corr[:64] >= 0).any() and (corr[128:192] >= 0).any() and (corr[192:] >= 0).any()


def test_none_has_no_correspondence():
    G, cnt = pc.info_oracle("none")
    assert cnt == 0 and not G.any() and (_corr("none") < 0).all()


def test_ties_pick_the_lower_index():
    S, T, d, _ = pc.info_case("ties")
    corr = _corr("ties")
    tied = lower_x = 0
    for i in range(len(S)):
        e = S[i] - T
        d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        best = np.flatnonzero(d2 == d2.min())
        assert d2.min() < d * d and corr[i] == best[0]
        tied += len(best) == 2
        lower_x += len(best) == 2 and T[corr[i], 0] < S[i, 0]
    # (the lattice's last column has one nearest target); the lower index lies on either side
    assert tied == 24 * 23 and 200 < lower_x < tied - 200


def test_anchored_targets_take_the_sparse_table_and_wide_cells():
    for name, wide in (("anchors_2e4", False), ("anchors_1e7", True)):
        _, T, d, _ = pc.info_case(name)
        edge, count = rc.grid_cells(T, d)
        assert count > rc.DENSE_CELLS and (edge > d) == wide
        assert pc.info_oracle(name)[1] > 0


def test_registration_pairs_follow_the_reference_loop():
    assert po.registration_pairs(2) == [(0, 1)]
    assert po.registration_pairs(4) == [(0, 1), (0, 3), (1, 2), (2, 3)]


def test_vec6_inverts_mat_and_the_singular_graph_takes_the_other_branch():
    v = [0.3, -0.4, 1.1, 1.0, -2.0, 3.0]
    assert np.allclose(po.vec6(po.mat(v)), v, rtol=0, atol=1e-15)
    init, _, truth = pc.graph_case("singular")
    for nodes in (init, truth):
        sy = [math.sqrt(T[0][0] ** 2 + T[1][0] ** 2) for T in nodes]
        assert sy[0] < 1e-6 and all(s >= 1e-6 for s in sy[1:])
    assert po.vec6(po._m(truth[0]))[2] == 0.0


@pytest.mark.parametrize("name", pc.GRAPH_CASES)
def test_graph_edges_are_exact_for_the_ground_truth_and_not_for_the_start(name):
    init, edges, truth = pc.graph_case(name)
    assert np.array_equal(init[0], truth[0])
    assert po.graph_residual([po._m(T) for T in truth], [(s, t, po._m(X), L.tolist()) for s, t, X, L in edges]) < 1e-20
    nodes, info = pc.graph_oracle(name)
    assert info["initial_residual"] > 1.0 > info["final_residual"]
    assert [(s, t) for s, t, _, _ in edges] == po.registration_pairs(len(truth))
