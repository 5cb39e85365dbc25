"""Host-side helpers of the per-entry missing-data prediction paths (predict_missing_data(..., observed=...) of bayesian_gp_lvm
and dp_gp_lvm).  NumPy only; not on the hot path, importable without a GPU."""
import numpy as np


def observed_mask(y):
    """Boolean [N* x D]: True where y holds a measurement (not NaN)."""
    return ~np.isnan(np.asarray(y, dtype=np.float64))


def check_observed(observed, shape):
    """The mask as a boolean array after the argument checks shared by the models (AssertionError on a non-boolean mask or a
    shape other than `shape`)."""
    observed = np.asarray(observed)
    assert observed.dtype == np.bool_, 'observed must be a boolean array'
    assert observed.ndim == 2 and tuple(observed.shape) == tuple(shape), 'observed must have the shape of y_test, [N* x D]'
    return observed


def zero_filled(y, observed):
    """y with every unobserved entry (NaN or not) replaced by 0."""
    return np.where(observed, np.asarray(y, dtype=np.float64), 0.0)


def masked_arguments(y_test, observed, num_dimensions, predict=False, reference_compat=False):
    """The argument checks of the models' observed= paths; returns (y_test zero-filled where unobserved [N* x D], the mask).
    predict: a mask that is True everywhere is refused (nothing would be predicted)."""
    assert not reference_compat, 'reference_compat has no meaning with observed: the reference has no per-entry masks'
    y_test = np.asarray(y_test, dtype=np.float64)
    assert y_test.ndim == 2 and y_test.shape[0] >= 1 and y_test.shape[1] == num_dimensions, \
        'with observed, y_test must be [N* x D]'
    observed = check_observed(observed, y_test.shape)
    assert observed.any(), 'observed must hold at least one True entry'
    if predict:
        assert not observed.all(), 'observed is True everywhere: nothing is missing (use predict_new_latent_variables)'
    return zero_filled(y_test, observed), observed


def group_columns_by_pattern(observed):
    """Column groups of a boolean mask [N* x D] that share one row pattern: a list of (columns ascending [int array],
    row_weights [N*] float64 of 0 / 1), ordered by each group's first column; columns with no observed entry are left out."""
    observed = np.asarray(observed)
    assert observed.dtype == np.bool_ and observed.ndim == 2, 'observed must be a boolean [N* x D] array'
    groups, index = [], {}
    for d in range(observed.shape[1]):
        col = observed[:, d]
        if not col.any():
            continue
        key = np.packbits(col).tobytes()
        if key not in index:
            index[key] = len(groups)
            groups.append(([], col.astype(np.float64)))
        groups[index[key]][0].append(d)
    return [(np.asarray(cols, dtype=np.int64), w) for cols, w in groups]


def observed_columns(observed, lo=0, hi=None):
    """The columns among [lo, hi) (default: all) with at least one observed entry, ascending, counted from `lo`: the operator batch
    of a masked over-D bound on that share of the columns (a D-sharded model: lo, hi = the rank's bounds).  May be empty; the
    batches of the shares of a partition of [0, D), each shifted by its lo, make up the batch of the whole mask."""
    observed = np.asarray(observed)
    return np.flatnonzero(observed[:, lo:hi].any(axis=0))


def missing_columns(observed):
    """Columns with at least one unobserved entry, ascending."""
    return np.flatnonzero(~np.asarray(observed).all(axis=0))


def masked_nearest_neighbour(y_train, y_test, observed):
    """For every test row, the index of the training row with the smallest mean squared difference over that row's observed
    columns (for a mask that is the first Do columns in every row: the nearest neighbour over y_train[:, :Do]); -1 for a row
    with nothing observed."""
    y_train = np.asarray(y_train, dtype=np.float64)
    y_test = zero_filled(y_test, observed)
    out = np.full(y_test.shape[0], -1, dtype=np.int64)
    for n in range(y_test.shape[0]):
        cols = np.flatnonzero(observed[n])
        if cols.size:
            out[n] = np.argmin(np.mean((y_train[:, cols] - y_test[n, cols][None, :]) ** 2, axis=1))
    return out


def masked_nearest_neighbour_init(y_train, y_test, observed, x_train_mean):
    """Initial q(X*) means [N* x Q]: the training latent mean of masked_nearest_neighbour's row, the prior mean 0 for a test
    row with nothing observed, plus the N(0, 0.01^2) noise of the unmasked initialisation (one draw of the same shape from
    NumPy's global generator)."""
    x_train_mean = np.asarray(x_train_mean, dtype=np.float64)
    idx = masked_nearest_neighbour(y_train, y_test, observed)
    init = np.where((idx >= 0)[:, None], x_train_mean[np.maximum(idx, 0)], 0.0)
    return init + np.random.normal(scale=0.01, size=init.shape)


def column_mean_filled(y, observed):
    """y with every unobserved entry replaced by the mean of its column's observed entries (0 for a column never observed):
    the complete matrix whose PCA starts q(X) when bayesian_gp_lvm trains on data with missing entries."""
    observed = np.asarray(observed)
    y0 = zero_filled(y, observed)
    count = observed.sum(axis=0)
    mean = np.where(count > 0, y0.sum(axis=0) / np.maximum(count, 1), 0.0)
    return np.where(observed, y0, mean[None, :])


def jointly_observed_nearest_neighbour(y_train, train_observed, y_test, test_observed):
    """For every test row, the index of the training row with the smallest mean squared difference over the columns observed
    in BOTH rows; training rows that share no observed column with the test row are skipped; -1 for a test row with no
    candidate (the nearest neighbour of a model trained on data with missing entries)."""
    train_observed, test_observed = np.asarray(train_observed), np.asarray(test_observed)
    y_train, y_test = zero_filled(y_train, train_observed), zero_filled(y_test, test_observed)
    out = np.full(y_test.shape[0], -1, dtype=np.int64)
    for n in range(y_test.shape[0]):
        both = train_observed & test_observed[n][None, :]
        count = both.sum(axis=1)
        if not count.any():
            continue
        total = np.where(both, (y_train - y_test[n][None, :]) ** 2, 0.0).sum(axis=1)
        out[n] = np.argmin(np.where(count > 0, total / np.maximum(count, 1), np.inf))
    return out


def jointly_observed_nearest_neighbour_init(y_train, train_observed, y_test, test_observed, x_train_mean):
    """Initial q(X*) means [N* x Q] as masked_nearest_neighbour_init, from jointly_observed_nearest_neighbour's row (the prior
    mean 0 for a test row with no candidate)."""
    x_train_mean = np.asarray(x_train_mean, dtype=np.float64)
    idx = jointly_observed_nearest_neighbour(y_train, train_observed, y_test, test_observed)
    init = np.where((idx >= 0)[:, None], x_train_mean[np.maximum(idx, 0)], 0.0)
    return init + np.random.normal(scale=0.01, size=init.shape)
