"""Host tests (no GPU) of the two helpers of utils/missing.py behind bayesian_gp_lvm(..., observed=...): the column-mean fill
that starts q(X), and the nearest training neighbour over jointly observed columns that starts q(X*) on a mask-trained model."""
import numpy as np

from dp_gp_lvm_amd.utils import missing

NAN = np.nan


def test_column_mean_fill_with_a_never_observed_column():
    y = np.array([[1.0, NAN, 3.0, 7.0],
                  [3.0, NAN, NAN, 7.0],
                  [NAN, NAN, 5.0, 1.0]])
    obs = missing.observed_mask(y)
    got = missing.column_mean_filled(y, obs)
    want = np.array([[1.0, 0.0, 3.0, 7.0],
                     [3.0, 0.0, 4.0, 7.0],
                     [2.0, 0.0, 5.0, 1.0]])
    np.testing.assert_array_equal(got, want)
    # unobserved entries are ignored whatever they hold
    np.testing.assert_array_equal(missing.column_mean_filled(np.where(obs, y, 99.0), obs), want)
    full = np.arange(6.0).reshape(2, 3)
    np.testing.assert_array_equal(missing.column_mean_filled(full, np.ones((2, 3), dtype=bool)), full)


def test_jointly_observed_nearest_neighbour():
    y_train = np.array([[0.0, 0.0, NAN],        # shares columns 0, 1 with test row 0
                        [NAN, NAN, 9.0],        # shares no column with test row 0: skipped, though its zero fill is closest
                        [1.0, 5.0, 2.0],
                        [1.1, NAN, NAN]])
    train_obs = missing.observed_mask(y_train)
    y_test = np.array([[1.0, 0.2, NAN],
                       [NAN, NAN, 8.0],
                       [NAN, NAN, NAN]])        # nothing observed: no candidate
    test_obs = missing.observed_mask(y_test)
    idx = missing.jointly_observed_nearest_neighbour(y_train, train_obs, y_test, test_obs)
    # row 0: means over the shared columns are 0.52 (train 0), 11.52 (train 2), 0.01 (train 3, column 0 only)
    np.testing.assert_array_equal(idx, [3, 1, -1])
    # a test row whose only observed column no training row observed has no candidate either
    train_obs2 = train_obs.copy()
    train_obs2[:, 2] = False
    idx = missing.jointly_observed_nearest_neighbour(y_train, train_obs2, y_test, test_obs)
    np.testing.assert_array_equal(idx, [3, -1, -1])
    x_train = np.arange(8.0).reshape(4, 2) + 1.0
    np.random.seed(0)
    init = missing.jointly_observed_nearest_neighbour_init(y_train, train_obs, y_test, test_obs, x_train)
    assert np.abs(init[0] - x_train[3]).max() < 0.06 and np.abs(init[1] - x_train[1]).max() < 0.06
    assert np.abs(init[2]).max() < 0.06          # the prior mean for the row with no candidate
    # with both masks True everywhere it is the plain nearest neighbour
    rs = np.random.default_rng(1)
    a, b = rs.standard_normal((7, 3)), rs.standard_normal((4, 3))
    want = np.argmin(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1), axis=0)
    np.testing.assert_array_equal(
        missing.jointly_observed_nearest_neighbour(a, np.ones(a.shape, dtype=bool), b, np.ones(b.shape, dtype=bool)), want)
