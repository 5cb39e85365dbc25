"""Where is the middle of a group of latent points, measured along the data manifold?

Synthetic data (utils.synthetic.grouped_outputs): D = 18 output dims in three blocks, each a function of two of three latent
coordinates.  The over-T DP-GP-LVM (T = 4 atoms) is trained on it; then, under the metric of the output dims of one group the DP
discovered (argmax of q(Z), the largest group), the Frechet mean of `points` training latents is found by Riemannian gradient
descent,
    mu <- exp_mu(eta mean_i log_mu(x_i)),
with model.latent_log_map (Newton shooting on the discrete exponential map, exact Jacobian) and model.latent_exp_map.  Printed: per
descent step the sum of squared geodesic distances sum_i |log_mu(x_i)|_G^2 and the Riemannian norm of the mean logarithm (the
gradient: it goes to zero at the Frechet mean); then the Frechet mean and its sum of squares against those of the Euclidean mean of
the same points; and, for the pairs (Frechet mean, x_i), the energy of the logarithm map's curve beside that of
model.latent_geodesic (200 Adam iterations on a polyline) between the same ends, with the logarithm map's end residual.

    python examples/latent_log_map.py [--iterations 300] [--points 12] [--steps 32] [--descent 8] [--eta 1.0] [--seed 1]
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
    ap.add_argument('--points', type=int, default=12)
    ap.add_argument('--steps', type=int, default=32)
    ap.add_argument('--descent', type=int, default=8)
    ap.add_argument('--eta', type=float, default=1.0)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--integrator', choices=('host', 'device'), default='host', help='where the Runge-Kutta loops run')
    args = ap.parse_args()
    np.random.seed(args.seed)
    y, _, block = synthetic.grouped_outputs(120, 18, seed=args.seed)
    q = 4
    model = dp_gp_lvm_t(y, num_latent_dims=q, num_inducing_points=20, truncation_level=4)
    model.integrator = args.integrator
    model.optimise(args.iterations, learning_rate=0.05)
    x_mean = model.q_x[0].detach()
    group = model.assignments.detach().cpu().numpy().argmax(axis=1)
    biggest = np.bincount(group).argmax()
    cols = np.flatnonzero(group == biggest)
    pick = np.random.default_rng(args.seed).permutation(x_mean.shape[0])[:args.points]
    pts = x_mean[torch.as_tensor(pick, device=x_mean.device)].contiguous()
    n = pts.shape[0]
    print('group %d: %d dims (true blocks %s); %d training latents, %d steps per geodesic'
          % (biggest, cols.size, sorted(set(block[cols].tolist())), n, args.steps))

    def logs(mu):
        """(log_mu(x_i) [n x Q], squared distances [n], curves, residuals) at the point mu [Q]."""
        v, dist, curve, res = model.latent_log_map(mu[None].expand(n, q), pts, num_steps=args.steps, columns=cols)
        return v, dist * dist, curve, res

    euclid = pts.mean(dim=0)
    mu = euclid.clone()
    for it in range(args.descent):
        v, d2, _, res = logs(mu)
        grad = v.mean(dim=0)
        g = model.latent_metric(mu[None], columns=cols)[0]
        print('    step %d: sum of squared distances %.6f, |mean log|_G %.3e, largest end residual %.1e'
              % (it, float(d2.sum()), float(torch.sqrt(grad @ g @ grad)), float(res.max())))
        mu = model.latent_exp_map(mu, args.eta * grad, num_steps=args.steps, columns=cols)[-1]
    v, d2, curve, res = logs(mu)
    _, d2_e, _, _ = logs(euclid)
    fmt = lambda t: '[' + ', '.join('%.4f' % float(a) for a in t) + ']'
    print('Frechet mean   %s: sum of squared geodesic distances %.6f' % (fmt(mu), float(d2.sum())))
    print('Euclidean mean %s: sum of squared geodesic distances %.6f; the two means are %.4f apart'
          % (fmt(euclid), float(d2_e.sum()), float((mu - euclid).norm())))
    e_log = model.curve_energy(curve, columns=cols)
    _, _, e_adam = model.latent_geodesic(mu[None].expand(n, q), pts, num_segments=args.steps, columns=cols)
    print('curve energy from the Frechet mean, logarithm map against latent_geodesic (200 Adam iterations):')
    for i in range(n):
        print('    latent %3d: log map %.6f (|v|_G^2 %.6f, end residual %.1e), latent_geodesic %.6f'
              % (int(pick[i]), float(e_log[i]), float(d2[i]), float(res[i]), float(e_adam[i])))
    print('    sum: log map %.6f, latent_geodesic %.6f' % (float(e_log.sum()), float(e_adam.sum())))


if __name__ == '__main__':
    main()
