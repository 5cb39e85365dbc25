"""Starting at a latent point in a given direction, where does the data manifold take you?

Synthetic data (utils.synthetic.grouped_outputs): D = 18 output dims in three blocks, each a function of two of three latent
coordinates.  The over-T DP-GP-LVM (T = 4 atoms) is trained on it; then a fan of geodesics is shot from one training latent
(model.latent_exp_map: the exponential map under the expected metric G, Tosi et al., UAI 2014) in `rays` directions of the plane of
the two most relevant latent dims, each with the same Riemannian speed |v|_G, once under the metric of all output dims and once
under the metric of the dims of every group the DP discovered (argmax of q(Z); the DP may keep a single group: then the rows
agree).  Printed per metric and ray: the curve_length of the geodesic against |v|_G (a geodesic has constant speed: they agree up
to the discretisation) and the largest predictive variance (model.predictive_marginals at x_var = 0, averaged over the dims) met
along the geodesic fan against the straight fan x + t v, with the distance between the two fans' ends (at a small radius the fan
stays inside the data and the two barely differ; raise --radius to see the geodesics bend).

    python examples/latent_exp_map.py [--iterations 300] [--rays 8] [--steps 64] [--radius 3.0] [--seed 1]
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
    ap.add_argument('--rays', type=int, default=8)
    ap.add_argument('--steps', type=int, default=64)
    ap.add_argument('--radius', type=float, default=3.0, help='the Riemannian length |v|_G of every ray')
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--integrator', choices=('host', 'device'), default='host', help='where the Runge-Kutta loop runs')
    args = ap.parse_args()
    np.random.seed(args.seed)
    y, _, block = synthetic.grouped_outputs(120, 18, seed=args.seed)
    q = 4
    model = dp_gp_lvm_t(y, num_latent_dims=q, num_inducing_points=20, truncation_level=4)
    model.integrator = args.integrator
    model.optimise(args.iterations, learning_rate=0.05)
    x_mean = model.q_x[0].detach()
    centre = torch.argmin(((x_mean - x_mean.mean(dim=0)) ** 2).sum(dim=1))            # the training latent nearest the middle
    x0 = x_mean[centre]
    plane = torch.argsort(x_mean.var(dim=0), descending=True)[:2]                      # the two latent dims the data spread over
    angle = torch.arange(args.rays, dtype=x0.dtype, device=x0.device) * (2.0 * np.pi / args.rays)
    dirs = torch.zeros((args.rays, q), dtype=x0.dtype, device=x0.device)
    dirs[:, plane[0]], dirs[:, plane[1]] = torch.cos(angle), torch.sin(angle)
    group = model.assignments.detach().cpu().numpy().argmax(axis=1)
    sets = [('all', np.arange(y.shape[1]))] + [('group%d' % t, np.flatnonzero(group == t)) for t in np.unique(group)]
    t = torch.linspace(0.0, 1.0, args.steps + 1, dtype=x0.dtype, device=x0.device)

    def worst_variance(curve, cols):
        pts = curve.reshape(-1, q)
        _, var = model.predictive_marginals(pts, torch.zeros_like(pts), columns=cols)
        return var.mean(dim=1).reshape(curve.shape[0], -1).max(dim=1)[0].cpu().numpy()

    for name, cols in sets:
        g = model.latent_metric(x0[None], columns=cols)[0]
        speed = torch.sqrt(torch.einsum('nq,qr,nr->n', dirs, g, dirs))
        v = dirs * (args.radius / speed)[:, None]                                      # every ray: |v|_G = radius
        start = x0[None].expand(args.rays, q)
        fan = model.latent_exp_map(start, v, num_steps=args.steps, columns=cols)
        straight = start[:, None, :] + t[None, :, None] * v[:, None, :]
        length = model.curve_length(fan, columns=cols)
        var_geo, var_line = worst_variance(fan, cols), worst_variance(straight, cols)
        print('%-7s %2d dims (true blocks %s), from latent %d' % (name, cols.size, sorted(set(block[cols].tolist())), int(centre)))
        for i in range(args.rays):
            print('    ray %2d (%5.1f deg): |v|_G %.4f, curve_length %.4f; end %.3f from the straight end; largest predictive '
                  'variance along the geodesic %.4f, along the straight ray %.4f'
                  % (i, float(angle[i]) * 180.0 / np.pi, args.radius, length[i], float((fan[i, -1] - straight[i, -1]).norm()),
                     var_geo[i], var_line[i]))
        print('    fan: largest predictive variance geodesic %.4f, straight %.4f' % (var_geo.max(), var_line.max()))


if __name__ == '__main__':
    main()
