"""Finding q(X*) from a few given columns by fitting the held-out predictive density, through a frozen predictor.

The latent points of a utils.synthetic problem (N = 80, Q = 2) are pushed through a smooth map to D = 8 columns (the problem's own y
is white noise and has nothing to predict).  A bayesian_gp_lvm is trained on 60 rows.  Of the other 20 rows only 3 columns are
given.  model.frozen_predictor() builds the training side once; q(X*) = (x, softplus(raw)) is then found by Adam on the negative log
predictive density of the given entries, -sum log N(y | mean(x, s), var(x, s)), differentiated through p(x, s) (the backward pass is
the HIP adjoint of the moments, ops.qx_psi_point_moments_adjoint).  Printed: the RMSE on the 5 columns that were NOT given next to
the RMSE of predicting the training column means, and the share of those entries within two predictive standard deviations.

    python examples/latent_targets.py [--iterations 300] [--steps 150] [--seed 3]
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dp_gp_lvm_amd.models.gaussian_process import bayesian_gp_lvm   # noqa: E402
from dp_gp_lvm_amd.models.predictor import negative_log_density      # noqa: E402
from dp_gp_lvm_amd.utils.synthetic import make_problem               # noqa: E402

GIVEN = [0, 3, 6]


def data(seed):
    x = make_problem(shape=(80, 8, 12, 2), seed=seed)['mu']
    rs = np.random.default_rng(seed + 1)
    y = np.concatenate([np.sin(x), np.cos(x)], axis=1) @ rs.standard_normal((4, 8)) + 0.05 * rs.standard_normal((80, 8))
    y = (y - y[:60].mean(axis=0)) / y[:60].std(axis=0)
    return y[:60], y[60:]


def fit(p, y, given, x0, steps, learning_rate=0.05):
    """Adam on the held-out negative log density; returns (x_mean, x_var, first loss, last loss)."""
    xt = x0.clone().requires_grad_(True)
    raw = torch.zeros_like(xt).requires_grad_(True)              # x_var = softplus(raw)
    opt = torch.optim.Adam([xt, raw], lr=learning_rate)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = negative_log_density(*p(xt, F.softplus(raw)), y, given)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return xt.detach(), F.softplus(raw).detach(), losses[0], losses[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iterations', type=int, default=300)
    ap.add_argument('--steps', type=int, default=150)
    ap.add_argument('--seed', type=int, default=3)
    args = ap.parse_args()
    y_train, y_new = data(args.seed)
    model = bayesian_gp_lvm(y_train, num_latent_dims=2, num_inducing_points=12,
                            initial_values=dict(gamma=np.ones((1, 2)), alpha=1.0, beta=1.0))
    model.optimise(args.iterations, learning_rate=0.05)
    p = model.frozen_predictor()                                 # the training side, once (stale if the model trains on)
    x_train = model.raw_variables['x_mean'].detach()
    dev = x_train.device
    y = torch.as_tensor(y_new, device=dev)
    given = torch.zeros(y.shape, dtype=torch.bool, device=dev)
    given[:, GIVEN] = True
    # start at the latent point of the nearest training row over the given columns
    near = np.argmin(((y_new[:, None, GIVEN] - y_train[None, :, GIVEN]) ** 2).sum(axis=-1), axis=1)
    x0 = x_train[torch.as_tensor(near, device=dev)].to(torch.float64)
    x_mean, x_var, first, last = fit(p, y, given, x0, args.steps)
    mean, var = p(x_mean, x_var)
    rest = ~given
    err = (mean - y)[rest]
    print('held-out negative log density of the %d given entries: %.3f -> %.3f after %d Adam steps' % (int(given.sum()), first, last,
                                                                                                      args.steps))
    print('the %d entries that were not given: RMSE %.4f (column means: %.4f); share within 2 predictive standard deviations %.3f'
          % (int(rest.sum()), float(torch.sqrt(torch.mean(err ** 2))), float(np.sqrt(np.mean(y_new[:, [c for c in range(8) if c not in GIVEN]] ** 2))),
             float(torch.mean((err.abs() <= 2.0 * torch.sqrt(var[rest])).to(torch.float64)))))


if __name__ == '__main__':
    main()
