"""Train dp_gp_lvm (the over-D model) on data with missing entries and fill the gaps.

Synthetic data: D = 8 phase-shifted sines of one latent coordinate, 60 rows, 30 % of the entries removed at random.  The DP-GP-LVM
(T = 3 atoms, every column its own mixed kernel) is trained on the incomplete matrix (observed=mask); impute_training_data()
replaces every gap by the posterior mean of its column and, with return_variance=True, gives the per-entry error bars.

    python examples/train_d_missing.py [--iterations 300] [--seed 5]
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
    ap.add_argument('--seed', type=int, default=5)
    args = ap.parse_args()
    rs = np.random.default_rng(args.seed)
    t = np.sort(rs.uniform(-2.5, 2.5, 60))
    y = np.sin(1.3 * t[:, None] + np.pi * np.arange(8)[None, :] / 8.0) + 0.05 * rs.standard_normal((60, 8))
    y_gaps = np.where(rs.random(y.shape) >= 0.3, y, np.nan)
    mask = missing.observed_mask(y_gaps)
    atoms = 3
    model = dp_gp_lvm(y_gaps, num_latent_dims=2, num_inducing_points=10, truncation_level=atoms, observed=mask,
                      initial_values=dict(x_var=np.full((60, 2), 0.5), gamma_atoms=np.ones((atoms, 2)),
                                            alpha_atoms=np.ones((atoms, 1)), beta_atoms=np.ones((atoms, 1))))
    before = float(model.objective)
    model.optimise(args.iterations, learning_rate=0.05)
    imputed, var = (a.cpu().numpy() for a in model.impute_training_data(return_variance=True))
    rmse = np.sqrt(np.mean((imputed[~mask] - y[~mask]) ** 2))
    rmse_mean = np.sqrt(np.mean((missing.column_mean_filled(y_gaps, mask)[~mask] - y[~mask]) ** 2))
    print('%d of %d entries missing' % ((~mask).sum(), mask.size))
    print('objective %.3f -> %.3f after %d iterations' % (before, float(model.objective), args.iterations))
    print('imputation RMSE over the missing entries: %.4f (column means: %.4f)' % (rmse, rmse_mean))
    inside = np.abs(imputed[~mask] - y[~mask]) <= 2.0 * np.sqrt(var[~mask])
    print('%.0f %% of the missing entries lie within two predictive standard deviations' % (100.0 * inside.mean()))


if __name__ == '__main__':
    main()
