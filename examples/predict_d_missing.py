"""Train dp_gp_lvm (the over-D model) on data with missing entries, then predict the missing entries of new, incomplete rows.

Synthetic data: D = 8 phase-shifted sines of one latent coordinate.  The DP-GP-LVM (T = 3 atoms, every column its own mixed kernel)
is trained on 60 rows with 30 % of their entries removed (observed=mask); 20 further rows arrive with 30 % of their entries missing.
optimise_test_latents(..., form='shared') fits q(X*) to what was measured on one copy of the inducing inputs
(models/frozen_bound_d.py) and predict_missing_data() returns the mean and variance of every entry of the columns that have gaps.

    python examples/predict_d_missing.py [--iterations 300] [--test-iterations 100] [--seed 5]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm                # noqa: E402
from dp_gp_lvm_amd.utils import missing                            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iterations', type=int, default=300)
    ap.add_argument('--test-iterations', type=int, default=100)
    ap.add_argument('--seed', type=int, default=5)
    args = ap.parse_args()
    rs = np.random.default_rng(args.seed)
    rows = lambda n: np.sin(1.3 * np.sort(rs.uniform(-2.5, 2.5, n))[:, None] + np.pi * np.arange(8)[None, :] / 8.0) + \
        0.05 * rs.standard_normal((n, 8))
    y, y_new = rows(60), rows(20)
    y_train = np.where(rs.random(y.shape) >= 0.3, y, np.nan)
    y_gaps = np.where(rs.random(y_new.shape) >= 0.3, y_new, np.nan)
    train_mask, mask = missing.observed_mask(y_train), missing.observed_mask(y_gaps)
    atoms = 3
    model = dp_gp_lvm(y_train, num_latent_dims=2, num_inducing_points=10, truncation_level=atoms, observed=train_mask,
                      initial_values=dict(x_var=np.full((60, 2), 0.5), gamma_atoms=np.ones((atoms, 2)),
                                          alpha_atoms=np.ones((atoms, 1)), beta_atoms=np.ones((atoms, 1))))
    model.optimise(args.iterations, learning_rate=0.05)
    x_mean, x_var = model.optimise_test_latents(y_gaps, args.test_iterations, learning_rate=0.05, observed=mask, form='shared')
    bound, _, _, mean, var = model.predict_missing_data(y_gaps, x_test_mean=x_mean, x_test_var=x_var, observed=mask)
    cols = model.missing_columns
    held = ~mask[:, cols]
    err = (mean.cpu().numpy() - y_new[:, cols])[held]
    sd = np.sqrt(var.cpu().numpy()[held])
    col_means = np.nanmean(y_train, axis=0)
    rmse_mean = np.sqrt(np.mean((np.broadcast_to(col_means, y_new.shape)[:, cols] - y_new[:, cols])[held] ** 2))
    print('training: %d of %d entries missing; test: %d of %d entries missing, in %d columns'
          % ((~train_mask).sum(), train_mask.size, held.sum(), mask.size, len(cols)))
    print('prediction lower bound %.3f after %d iterations on q(X*)' % (float(bound), args.test_iterations))
    print('RMSE over the missing test entries: %.4f (training column means: %.4f)' % (np.sqrt(np.mean(err ** 2)), rmse_mean))
    print('share of the missing test entries within 2 predictive standard deviations: %.3f (mean sd %.3f)'
          % (np.mean(np.abs(err) <= 2.0 * sd), sd.mean()))


if __name__ == '__main__':
    main()
