"""What does the model say the outputs do along a path in latent space: not a mean and a band per point, but whole trajectories?

The data and the over-T DP-GP-LVM (T = 4 atoms) of examples/latent_geodesic.py.  One pair of training latents is joined by the
straight line and by the geodesic under the expected metric (model.latent_geodesic); along both paths model.sample_functions draws
five output trajectories from the JOINT posterior of the path's 33 points (model.predictive_covariance is its covariance), once for
all output dims and once for the dims of one group the DP discovered.  Printed per path and set of dims, with
roughness = the summed squared second differences along the path, averaged over the dims:
    the roughness of the mean path (model.predictive_marginals at x_var = 0),
    the roughness of a trajectory drawn from the joint posterior (the mean over the five draws),
    the roughness of five draws taken point by point from the marginals, mean + sqrt(var) xi with independent xi:
        white noise around the mean, not a function: this is what the joint covariance buys.
Both kinds of draws are noise-free functions (the marginals' 1/beta is taken out) and use the same standard normal numbers.

    python examples/latent_samples.py [--iterations 300] [--segments 32] [--geodesic-iterations 200] [--samples 5] [--seed 1]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm_t              # noqa: E402
from dp_gp_lvm_amd.utils import synthetic                          # noqa: E402


def roughness(f):
    """[...]: summed squared second differences along the path (axis -2) of f [... x N* x J], averaged over the J dims."""
    d2 = f[..., 2:, :] - 2.0 * f[..., 1:-1, :] + f[..., :-2, :]
    return (d2 * d2).sum(dim=-2).mean(dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iterations', type=int, default=300)
    ap.add_argument('--segments', type=int, default=32)
    ap.add_argument('--geodesic-iterations', type=int, default=200)
    ap.add_argument('--samples', type=int, default=5)
    ap.add_argument('--seed', type=int, default=1)
    args = ap.parse_args()
    np.random.seed(args.seed)
    y, _, block = synthetic.grouped_outputs(120, 18, seed=args.seed)
    q = 4
    model = dp_gp_lvm_t(y, num_latent_dims=q, num_inducing_points=20, truncation_level=4)
    model.optimise(args.iterations, learning_rate=0.05)
    x_mean = model.q_x[0].detach()
    pick = np.random.default_rng(args.seed).permutation(y.shape[0])[:2]
    a, b = x_mean[pick[:1]], x_mean[pick[1:]]
    group = model.assignments.detach().cpu().numpy().argmax(axis=1)
    first = np.unique(group)[0]
    sets = [('all', np.arange(y.shape[1])), ('group%d' % first, np.flatnonzero(group == first))]
    line, _, _ = model.latent_geodesic(a, b, num_segments=args.segments, num_iterations=0)
    geo, _, _ = model.latent_geodesic(a, b, num_segments=args.segments, num_iterations=args.geodesic_iterations)

    print('latents %d -> %d, %d points per path, %d draws' % (pick[0], pick[1], args.segments + 1, args.samples))
    for path_name, curve in (('straight line', line[0]), ('geodesic', geo[0])):
        for name, cols in sets:
            gen = torch.Generator(device=curve.device)
            gen.manual_seed(args.seed)
            xi = torch.randn((args.samples, curve.shape[0], cols.size), generator=gen, dtype=curve.dtype, device=curve.device)
            mean, var = model.predictive_marginals(curve, torch.zeros_like(curve), columns=cols)
            cov = model.predictive_covariance(curve, columns=cols)                         # [J, N*, N*], noise-free
            joint = model.sample_functions(curve, columns=cols, draws=xi, seed=args.seed)    # [S, N*, J]
            noise_free = torch.diagonal(cov, dim1=1, dim2=2).transpose(0, 1).clamp(min=0.0)    # the marginals' variance less 1/beta
            pointwise = mean[None] + torch.sqrt(noise_free)[None] * xi
            print('%-13s %-7s %2d dims (true blocks %s): roughness of the mean path %.4f, of a joint trajectory %.4f, of '
                  'independent draws from the marginals %.4f   (mean marginal variance %.4f, of which noise %.4f)'
                  % (path_name, name, cols.size, sorted(set(block[cols].tolist())), float(roughness(mean)),
                     float(roughness(joint).mean()), float(roughness(pointwise).mean()), float(var.mean()),
                     float((var - noise_free).mean())))


if __name__ == '__main__':
    main()
