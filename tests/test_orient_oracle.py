"""tests/orient_oracle.py on its own (no GPU): the restated orientation does what
it is for on a surface where the radial orientation fails, its forest is a
minimum one, and the result does not depend on the signs that come in."""
import numpy as np
import pytest

from tests import orient_oracle as oo


@pytest.fixture(scope="module", params=[0, 1, 2, 3])
def scrambled_torus(request):
    seed = request.param
    P, out = oo.torus(2000, seed)
    sign = np.random.default_rng(100 + seed).choice([-1.0, 1.0], size=(len(P), 1))
    idx, cnt = oo.hybrid(P, 0.3, 12)
    return P, out, out * sign, idx, cnt


def test_torus_is_oriented_outwards(scrambled_torus):
    P, out, N, idx, cnt = scrambled_torus
    got, tree, comps = oo.orient(P, N, idx, cnt)
    assert comps == 1 and len(tree) == 1999 and len(np.unique(tree)) == 1999
    assert np.array_equal(np.abs(got), np.abs(N))
    assert oo.agreement(got, out) == 1.0


def test_radial_orientation_fails_on_the_torus(scrambled_torus):
    P, out, N, _, _ = scrambled_torus
    share = oo.agreement(oo.radial(P, N), out)
    print(f"radial orientation agrees with the outward normal on {100 * share:.1f} % of the torus")
    assert 0.5 < share < 0.8


def _prim_weight(n, u, v, w):
    """Total weight of a minimum spanning forest by Prim over a dense matrix."""
    W = np.full((n, n), np.inf)
    np.minimum.at(W, (u, v), w)
    W = np.minimum(W, W.T)
    done = np.zeros(n, bool)
    total = 0.0
    for s in range(n):
        if done[s]:
            continue
        done[s] = True
        best = W[s].copy()
        while True:
            best[done] = np.inf
            t = int(np.argmin(best))
            if not np.isfinite(best[t]):
                break
            total += best[t]
            done[t] = True
            best = np.minimum(best, W[t])
    return total


@pytest.mark.parametrize("n,k,radius", [(300, 6, 0.45), (200, 3, 0.5), (120, 20, 0.6)])
def test_forest_is_minimal_and_signs_do_not_matter(n, k, radius):
    rng = np.random.default_rng(n)
    P, out = oo.torus(n, n)
    N = out + 0.3 * rng.normal(size=out.shape)  # noisy, so the weights differ
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    idx, cnt = oo.hybrid(P, radius, k)
    got, tree, comps = oo.orient(P, N, idx, cnt)
    slot, u, v, w, _ = oo.edges(N, idx, cnt)
    assert len(tree) == n - comps
    mine = w[np.searchsorted(slot, tree)].sum()
    assert abs(mine - _prim_weight(n, u, v, w)) <= 1e-12 * max(1.0, mine)
    for trial in range(3):
        sign = rng.choice([-1.0, 1.0], size=(n, 1))
        again, tree2, comps2 = oo.orient(P, N * sign, idx, cnt)
        assert np.array_equal(again, got) and np.array_equal(tree2, tree) and comps2 == comps


def test_rules_on_small_graphs():
    # an isolated point and a pair: the root is the higher point, made to point up; the other follows the edge
    P = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 1.0], [9.0, 9.0, 9.0]])
    N = np.array([[0.0, 0.6, 0.8], [0.0, 0.0, -1.0], [0.0, 0.0, -1.0]])
    idx, cnt = oo.hybrid(P, 2.0, 4)
    got, tree, comps = oo.orient(P, N, idx, cnt)
    assert comps == 2 and tree.tolist() == [1]  # slot 1 = (0, idx[0][1]) = (0, 1)
    np.testing.assert_array_equal(got, [[0.0, 0.6, 0.8], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0]])
    # a dot of exactly 0 does not flip; a zero normal stays zero
    N = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0]])
    got, _, _ = oo.orient(P, N, idx, cnt)
    np.testing.assert_array_equal(got, N)
    # empty and single
    e = np.zeros((0, 3))
    got, tree, comps = oo.orient(e, e, np.zeros((0, 3), np.int32), np.zeros(0, np.int32))
    assert got.shape == (0, 3) and len(tree) == 0 and comps == 0
    got, tree, comps = oo.orient(P[:1], -N[1:2], np.zeros((1, 1), np.int32), np.ones(1, np.int32))
    assert comps == 1 and len(tree) == 0
    np.testing.assert_array_equal(got, [[0.0, 0.0, 1.0]])
