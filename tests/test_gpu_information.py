"""sl_information_matrix (csrc/slinfo.inl: one wave64 per block of 64 source
points) bit for bit against tests/posegraph_oracle.py -- the 36 entries and the
correspondence count -- at the smallest shapes that can break the kernel.  The
inputs come from tests/posegraph_cases.py; tests/test_posegraph_oracle.py proves
on the CPU that each one meets its precondition (a partial last block, a whole
block without a correspondence, ties, the sparse cell table, wide cells)."""
import numpy as np
import pytest

from tests import posegraph_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mg():
    from structured_light_for_3d_model_replication_amd import merge
    return merge


@pytest.mark.parametrize("name", pc.INFO_CASES)
def test_information_matrix_vs_oracle(mg, name):
    S, T, d, M = pc.info_case(name)
    want, want_n = pc.info_oracle(name)
    got, got_n = mg.get_information_matrix_from_point_clouds(S, T, d, M, info=True)
    print(name, "correspondences", got_n, "oracle", want_n)
    assert got.shape == (6, 6) and got.dtype == np.float64
    np.testing.assert_array_equal(got, want)
    assert got_n == want_n
    assert np.array_equal(got, got.T)
    assert got[3, 3] == got[4, 4] == got[5, 5] == got_n


def test_without_info_returns_the_matrix_alone(mg):
    S, T, d, M = pc.info_case("blob65_moved")
    got = mg.get_information_matrix_from_point_clouds(S, T, d, M)
    np.testing.assert_array_equal(got, pc.info_oracle("blob65_moved")[0])


def test_empty_source_and_empty_target_give_the_zero_matrix(mg):
    S, T, d, M = pc.info_case("blob65_moved")
    for s, t in ((np.zeros((0, 3)), T), (S, np.zeros((0, 3))), (np.zeros((0, 3)), np.zeros((0, 3)))):
        got, n = mg.get_information_matrix_from_point_clouds(s, t, d, M, info=True)
        assert n == 0 and got.shape == (6, 6) and not got.any()


def test_bad_arguments_raise(mg):
    S, T, d, M = pc.info_case("blob65_moved")
    for value in (np.nan, np.inf):
        bad = T.copy()
        bad[17, 1] = value
        with pytest.raises(ValueError, match="non-finite target coordinates"):
            mg.get_information_matrix_from_point_clouds(S, bad, d, M)
    with pytest.raises(ValueError, match="max_correspondence_distance must be > 0"):
        mg.get_information_matrix_from_point_clouds(S, T, 0.0, M)
