"""Train manifold_relevance_determination on two views of which one is absent for a third of the rows, and fill the gaps.

Synthetic data: 60 rows of one latent coordinate; view 0 holds 8 phase-shifted sines, view 1 holds 5 phase-shifted cosines and
is missing altogether for 20 rows (a modality that was not recorded).  The model is trained on the incomplete views
(observed=[None, mask]) and impute_training_data() replaces every gap by its posterior mean: view 1 of the rows that lack it
is predicted from view 0 through the shared latent space.

    python examples/train_mrd_missing.py [--iterations 300] [--seed 5]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dp_gp_lvm_amd.models.gaussian_process import manifold_relevance_determination   # noqa: E402
from dp_gp_lvm_amd.utils import missing                                              # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iterations', type=int, default=300)
    ap.add_argument('--seed', type=int, default=5)
    args = ap.parse_args()
    rs = np.random.default_rng(args.seed)
    t = np.sort(rs.uniform(-2.5, 2.5, 60))
    view_0 = np.sin(1.3 * t[:, None] + np.pi * np.arange(8)[None, :] / 8.0) + 0.05 * rs.standard_normal((60, 8))
    view_1 = np.cos(0.9 * t[:, None] + np.pi * np.arange(5)[None, :] / 5.0) + 0.05 * rs.standard_normal((60, 5))
    gaps = view_1.copy()
    gaps[rs.permutation(60)[:20]] = np.nan
    mask = missing.observed_mask(gaps)
    np.random.seed(args.seed)                                # (the inducing inputs start at a random subset of the PCA)
    model = manifold_relevance_determination([view_0, gaps], num_latent_dims=2, num_inducing_points=10, observed=[None, mask],
                                             initial_values=dict(x_var=np.full((60, 2), 0.5), gamma=[np.ones((1, 2))] * 2,
                                                                 alpha=[1.0] * 2, beta=[1.0] * 2))
    before = float(model.objective)
    model.optimise(args.iterations, learning_rate=0.05)
    imputed = model.impute_training_data()[1].cpu().numpy()
    rmse = np.sqrt(np.mean((imputed[~mask] - view_1[~mask]) ** 2))
    rmse_mean = np.sqrt(np.mean((missing.column_mean_filled(gaps, mask)[~mask] - view_1[~mask]) ** 2))
    print('view 1 absent in %d of 60 rows' % (~mask).all(axis=1).sum())
    print('objective %.3f -> %.3f after %d iterations' % (before, float(model.objective), args.iterations))
    print('imputation RMSE over the missing entries of view 1: %.4f (column means: %.4f)' % (rmse, rmse_mean))


if __name__ == '__main__':
    main()
