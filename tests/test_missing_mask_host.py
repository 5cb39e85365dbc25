"""CPU tests (no GPU) of the host side of per-entry missing-data prediction (dp_gp_lvm_amd/utils/missing.py): the mask of a
NaN-filled array, the grouping of columns by row pattern, and the masked nearest-neighbour initialisation of q(X*)."""
import numpy as np
import pytest

from dp_gp_lvm_amd.utils import missing


def test_observed_mask():
    y = np.array([[1.0, np.nan, 0.0], [np.nan, np.nan, -2.0]])
    np.testing.assert_array_equal(missing.observed_mask(y), [[True, False, True], [False, False, True]])
    assert missing.observed_mask(y).dtype == np.bool_
    np.testing.assert_array_equal(missing.zero_filled(y, missing.observed_mask(y)), [[1.0, 0.0, 0.0], [0.0, 0.0, -2.0]])
    # an unobserved entry is ignored whatever it holds
    np.testing.assert_array_equal(missing.zero_filled([[5.0, 7.0]], np.array([[False, True]])), [[0.0, 7.0]])


def test_identical_columns_merge_and_groups_are_ordered_by_first_column():
    t, f = True, False
    obs = np.array([[t, f, t, t, f],
                    [t, t, t, f, t],
                    [f, t, f, f, t]])
    groups = missing.group_columns_by_pattern(obs)
    assert [list(c) for c, _ in groups] == [[0, 2], [1, 4], [3]]
    np.testing.assert_array_equal(groups[0][1], [1.0, 1.0, 0.0])
    np.testing.assert_array_equal(groups[1][1], [0.0, 1.0, 1.0])
    np.testing.assert_array_equal(groups[2][1], [1.0, 0.0, 0.0])
    assert all(w.dtype == np.float64 and w.shape == (3,) for _, w in groups)
    np.testing.assert_array_equal(missing.missing_columns(obs), [0, 1, 2, 3, 4])


def test_a_column_with_nothing_observed_is_dropped():
    obs = np.ones((4, 5), dtype=bool)
    obs[:, 1] = False
    obs[2, 3] = False
    groups = missing.group_columns_by_pattern(obs)
    assert [list(c) for c, _ in groups] == [[0, 2, 4], [3]]
    np.testing.assert_array_equal(groups[1][1], [1.0, 1.0, 0.0, 1.0])
    np.testing.assert_array_equal(missing.missing_columns(obs), [1, 3])
    assert missing.group_columns_by_pattern(np.zeros((3, 2), dtype=bool)) == []


def test_a_suffix_mask_is_one_group_of_all_ones():
    obs = np.zeros((6, 7), dtype=bool)
    obs[:, :4] = True
    (cols, w), = missing.group_columns_by_pattern(obs)
    np.testing.assert_array_equal(cols, [0, 1, 2, 3])
    np.testing.assert_array_equal(w, np.ones(6))
    np.testing.assert_array_equal(missing.missing_columns(obs), [4, 5, 6])


def test_mask_checks():
    with pytest.raises(AssertionError):
        missing.check_observed(np.ones((2, 3)), (2, 3))                    # not boolean
    with pytest.raises(AssertionError):
        missing.check_observed(np.ones((2, 3), dtype=bool), (2, 4))        # shape
    with pytest.raises(AssertionError):
        missing.group_columns_by_pattern(np.ones((2, 3), dtype=np.int64))
    assert missing.check_observed([[True, False]], (1, 2)).dtype == np.bool_


def test_masked_nearest_neighbour_of_a_suffix_mask_is_the_existing_initialisation():
    rs = np.random.default_rng(3)
    n, n_t, d, do, q = 40, 11, 8, 5, 3
    y_train, x_mean = rs.standard_normal((n, d)), rs.standard_normal((n, q))
    y_test = y_train[rs.integers(0, n, n_t)] + 0.05 * rs.standard_normal((n_t, d))
    obs = np.zeros((n_t, d), dtype=bool)
    obs[:, :do] = True
    y_nan = np.where(obs, y_test, np.nan)
    np.random.seed(5)
    have = missing.masked_nearest_neighbour_init(y_train, y_nan, obs, x_mean)
    # the unmasked initialisation of the models over y_train[:, :Do] (utils/expressions.py:28-44 of the reference), same seed
    np.random.seed(5)
    d2 = ((y_train[:, None, :do] - y_test[None, :, :do]) ** 2).sum(-1)
    want = x_mean[np.argmin(d2, axis=0)] + np.random.normal(scale=0.01, size=(n_t, q))
    np.testing.assert_array_equal(have, want)


def test_masked_nearest_neighbour_uses_each_rows_own_columns():
    y_train = np.array([[0.0, 0.0, 9.0], [5.0, 5.0, 0.0], [9.0, 0.0, 0.0]])
    x_mean = np.array([[1.0], [2.0], [3.0]])
    y_test = np.array([[np.nan, np.nan, 8.0], [4.0, 6.0, np.nan], [np.nan, np.nan, np.nan], [8.5, np.nan, 0.5]])
    obs = missing.observed_mask(y_test)
    np.testing.assert_array_equal(missing.masked_nearest_neighbour(y_train, y_test, obs), [0, 1, -1, 2])
    np.random.seed(0)
    init = missing.masked_nearest_neighbour_init(y_train, y_test, obs, x_mean)
    np.random.seed(0)
    noise = np.random.normal(scale=0.01, size=(4, 1))
    np.testing.assert_array_equal(init, np.array([[1.0], [2.0], [0.0], [3.0]]) + noise)     # nothing observed: 0 + noise
    assert np.all(noise != 0.0)
