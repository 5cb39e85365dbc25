"""Error bars on filled-in values from a bayesian_gp_lvm trained on data with gaps.

Synthetic data: D = 8 phase-shifted sines of one latent coordinate.  The model is trained on 60 rows with 30 % of their entries
missing (observed=mask); 20 further rows arrive with 30 % of their entries missing too.  optimise_test_latents() fits q(X*) to what
was measured of them and predictive_marginals() returns the mean and the variance of every entry, observation noise included.
Printed: the RMSE over the held-out entries, their mean log density under N(mean, var) and the share of them within two
predictive standard deviations; the same share for the gaps of the training data from impute_training_data(return_variance=True).

    python examples/predict_uncertainty.py [--iterations 300] [--test-iterations 100] [--seed 5]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dp_gp_lvm_amd.models.gaussian_process import bayesian_gp_lvm   # noqa: E402
from dp_gp_lvm_amd.utils import missing                            # noqa: E402


def report(tag, mean, var, truth, held):
    err, v = (mean - truth)[held], var[held]
    print('%s: %d held-out entries; RMSE %.4f; mean log density %.3f; share within 2 predictive standard deviations %.3f '
          '(mean sd %.3f)' % (tag, held.sum(), np.sqrt(np.mean(err ** 2)), np.mean(-0.5 * (np.log(2.0 * np.pi * v) + err ** 2 / v)),
                              np.mean(np.abs(err) <= 2.0 * np.sqrt(v)), np.sqrt(v).mean()))


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
    y_gaps, y_new_gaps = (np.where(rs.random(a.shape) >= 0.3, a, np.nan) for a in (y, y_new))
    mask, mask_new = missing.observed_mask(y_gaps), missing.observed_mask(y_new_gaps)
    model = bayesian_gp_lvm(y_gaps, num_latent_dims=2, num_inducing_points=10, observed=mask,
                            initial_values=dict(gamma=np.ones((1, 2)), alpha=1.0, beta=1.0))
    model.optimise(args.iterations, learning_rate=0.05)
    filled, var = model.impute_training_data(return_variance=True)
    report('training rows', filled.cpu().numpy(), var.cpu().numpy(), y, ~mask)
    x_mean, x_var = model.optimise_test_latents(y_new_gaps, args.test_iterations, learning_rate=0.05, observed=mask_new)
    mean, var = model.predictive_marginals(x_mean, x_var)
    report('new rows', mean.cpu().numpy(), var.cpu().numpy(), y_new, ~mask_new)


if __name__ == '__main__':
    main()
