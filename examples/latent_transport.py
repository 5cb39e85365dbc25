"""A latent analogy along the data manifold: "c is to ? as a is to b".

Synthetic data (utils.synthetic.grouped_outputs): D = 18 output dims in three blocks, each a function of two of three latent
coordinates.  The over-T DP-GP-LVM (T = 4 atoms) is trained on it; then, under the metric of the output dims of one group the DP
discovered (argmax of q(Z), the largest group), for three training latents a, b, c:
    u = log_a(b)                     model.latent_log_map
    u' = transport of u from a to c  model.latent_transport_to (parallel transport along the geodesic from a to c)
    d = exp_c(u')                    model.latent_exp_map
Printed: |u|_G at a and |u'|_G at c, which parallel transport keeps up to the integrator's error; the end point d beside the
Euclidean answer c + (b - a); and the Gram matrix <w_i, w_j>_G of a G-orthonormal frame at a after its transport to c, against
the identity.

    python examples/latent_transport.py [--iterations 300] [--steps 32] [--seed 1]
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
    ap.add_argument('--steps', type=int, default=32)
    ap.add_argument('--seed', type=int, default=1)
    args = ap.parse_args()
    np.random.seed(args.seed)
    y, _, block = synthetic.grouped_outputs(120, 18, seed=args.seed)
    q = 4
    model = dp_gp_lvm_t(y, num_latent_dims=q, num_inducing_points=20, truncation_level=4)
    model.optimise(args.iterations, learning_rate=0.05)
    x_mean = model.q_x[0].detach()
    group = model.assignments.detach().cpu().numpy().argmax(axis=1)
    biggest = np.bincount(group).argmax()
    cols = np.flatnonzero(group == biggest)
    pick = np.random.default_rng(args.seed).permutation(x_mean.shape[0])[:3]
    a, b, c = (x_mean[int(i)].contiguous() for i in pick)
    print('group %d: %d dims (true blocks %s); training latents a = %d, b = %d, c = %d; %d steps per geodesic'
          % (biggest, cols.size, sorted(set(block[cols].tolist())), pick[0], pick[1], pick[2], args.steps))
    norm = lambda x, w: float(torch.sqrt(w @ model.latent_metric(x[None], columns=cols)[0] @ w))
    fmt = lambda t: '[' + ', '.join('%.4f' % float(e) for e in t) + ']'

    u, dist, _, res = model.latent_log_map(a, b, num_steps=args.steps, columns=cols)
    moved, v_ac, dist_ac, res_ac = model.latent_transport_to(a, c, u, num_steps=args.steps, columns=cols)
    print('u = log_a(b) %s: |u|_G = %.8f at a (distance %.8f, end residual %.1e)' % (fmt(u), norm(a, u), float(dist), float(res)))
    print('u moved to c %s: |u|_G = %.8f at c (a to c: distance %.6f, end residual %.1e); relative change of the norm %.2e'
          % (fmt(moved), norm(c, moved), float(dist_ac), float(res_ac), abs(norm(c, moved) - norm(a, u)) / norm(a, u)))
    d = model.latent_exp_map(c, moved, num_steps=args.steps, columns=cols)[-1]
    flat = c + (b - a)
    print('analogy end exp_c(u at c) %s; Euclidean c + (b - a) %s; the two are %.4f apart (|b - a| = %.4f)'
          % (fmt(d), fmt(flat), float((d - flat).norm()), float((b - a).norm())))

    g = model.latent_metric(a[None], columns=cols)[0]
    frame = torch.linalg.inv(torch.linalg.cholesky(g)).contiguous()     # rows w_i = L^-1 e_i: w_i^T G w_j = (L^-1 G L^-T)_ij = delta_ij
    at_c = model.latent_parallel_transport(a[None], v_ac[None], frame[None], num_steps=args.steps, columns=cols)[0]
    gram = at_c @ model.latent_metric(c[None], columns=cols)[0] @ at_c.T
    start = frame @ g @ frame.T
    eye = torch.eye(q, dtype=gram.dtype, device=gram.device)
    print('Gram matrix of a G-orthonormal frame at a after its transport to c (|Gram - I| %.2e at a, %.2e at c):'
          % (float((start - eye).abs().max()), float((gram - eye).abs().max())))
    for row in gram:
        print('    ' + fmt(row))


if __name__ == '__main__':
    main()
