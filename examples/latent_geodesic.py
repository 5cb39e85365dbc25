"""How far apart are two latent points along the data manifold, and what path joins them?

Synthetic data (utils.synthetic.grouped_outputs): D = 18 output dims in three blocks, each a function of two of three latent
coordinates.  The over-T DP-GP-LVM (T = 4 atoms) is trained on it; then a few pairs of training latents are joined by the straight
line and by the geodesic under the expected metric G (model.latent_geodesic, Tosi et al., UAI 2014): once under the metric of all
output dims and once under the metric of the dims of every group the DP discovered (argmax of q(Z)): a group's geodesic length says
which points that group considers close (the DP may keep a single group: then the rows agree).  Printed per pair and metric: the
length of the straight line and of the geodesic under that metric, their energies, and the predictive variance
(model.predictive_marginals at x_var = 0) averaged along both paths: the geodesic stays where the model has seen data.

    python examples/latent_geodesic.py [--iterations 300] [--pairs 4] [--segments 32] [--geodesic-iterations 200] [--seed 1]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm_t              # noqa: E402
from dp_gp_lvm_amd.utils import synthetic                          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iterations', type=int, default=300)
    ap.add_argument('--pairs', type=int, default=4)
    ap.add_argument('--segments', type=int, default=32)
    ap.add_argument('--geodesic-iterations', type=int, default=200)
    ap.add_argument('--seed', type=int, default=1)
    args = ap.parse_args()
    np.random.seed(args.seed)
    y, _, block = synthetic.grouped_outputs(120, 18, seed=args.seed)
    q = 4
    model = dp_gp_lvm_t(y, num_latent_dims=q, num_inducing_points=20, truncation_level=4)
    model.optimise(args.iterations, learning_rate=0.05)
    x_mean = model.q_x[0].detach()
    pick = np.random.default_rng(args.seed).permutation(y.shape[0])[:2 * args.pairs]
    a, b = x_mean[pick[:args.pairs]], x_mean[pick[args.pairs:]]
    group = model.assignments.detach().cpu().numpy().argmax(axis=1)
    sets = [('all', np.arange(y.shape[1]))] + [('group%d' % t, np.flatnonzero(group == t)) for t in np.unique(group)]

    def mean_variance(curve, cols):
        pts = curve.reshape(-1, q)
        _, var = model.predictive_marginals(pts, torch.zeros_like(pts), columns=cols)
        return var.reshape(curve.shape[0], -1).mean(dim=1).cpu().numpy()

    for name, cols in sets:
        line, line_len, line_en = model.latent_geodesic(a, b, num_segments=args.segments, num_iterations=0, columns=cols)
        geo, geo_len, geo_en = model.latent_geodesic(a, b, num_segments=args.segments, num_iterations=args.geodesic_iterations,
                                                     columns=cols)
        var_line, var_geo = mean_variance(line, cols), mean_variance(geo, cols)
        print('%-7s %2d dims (true blocks %s)' % (name, cols.size, sorted(set(block[cols].tolist()))))
        for i in range(args.pairs):
            print('    latents %3d -> %3d: length straight %.4f, geodesic %.4f; energy straight %.4f, geodesic %.4f; '
                  'mean predictive variance straight %.4f, geodesic %.4f'
                  % (pick[i], pick[args.pairs + i], line_len[i], geo_len[i], line_en[i], geo_en[i], var_line[i], var_geo[i]))


if __name__ == '__main__':
    main()
