"""Where is the learnt map from latent space to data stretched, and by which outputs?

Synthetic data (utils.synthetic.grouped_outputs): D = 18 output dims in three blocks, each a function of two of three latent
coordinates.  The over-T DP-GP-LVM (T = 4 atoms) is trained on it; then the magnification factor sqrt(det G(x)) of the expected
metric G (model.magnification, Tosi et al., UAI 2014) is evaluated on a 2-D grid through the two most relevant latent dimensions
(the others at 0), once for all output dims and once for the dims of every group the DP discovered (argmax of q(Z)): a group's
grid shows which region and which latent directions that group uses (the DP may keep a single group: then the two grids agree).
Printed: one summary row per grid; saved: the grids as .npy files (no plotting library is used; any viewer of arrays will draw them).

    python examples/latent_magnification.py [--iterations 300] [--side 60] [--seed 1] [--out magnification]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm_t              # noqa: E402
from dp_gp_lvm_amd.utils import synthetic                          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iterations', type=int, default=300)
    ap.add_argument('--side', type=int, default=60)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--out', default='magnification')
    args = ap.parse_args()
    np.random.seed(args.seed)
    y, _, block = synthetic.grouped_outputs(120, 18, seed=args.seed)
    q = 4
    model = dp_gp_lvm_t(y, num_latent_dims=q, num_inducing_points=20, truncation_level=4)
    model.optimise(args.iterations, learning_rate=0.05)
    gamma, alpha, _ = (a.detach().cpu().numpy() for a in model.dp_atoms)
    phi = model.assignments.detach().cpu().numpy()                  # [D, T]
    relevance = (phi @ (alpha * gamma)).sum(axis=0)                 # sum_d sum_t phi_td alpha_t gamma_tq: the prior metric's diagonal
    qa, qb = np.sort(np.argsort(relevance)[-2:])
    x_mean = model.q_x[0].detach().cpu().numpy()
    lo, hi = x_mean[:, [qa, qb]].min(axis=0), x_mean[:, [qa, qb]].max(axis=0)
    grid = np.zeros((args.side * args.side, q))
    grid[:, qa] = np.repeat(np.linspace(lo[0], hi[0], args.side), args.side)
    grid[:, qb] = np.tile(np.linspace(lo[1], hi[1], args.side), args.side)
    print('latent relevance per dimension: %s; grid through dimensions %d and %d' % (np.round(relevance, 3), qa, qb))
    group = phi.argmax(axis=1)
    sets = [('all', np.arange(y.shape[1]))] + [('group%d' % t, np.flatnonzero(group == t)) for t in np.unique(group)]
    for name, cols in sets:
        mag = model.magnification(grid, columns=cols).cpu().numpy().reshape(args.side, args.side)
        g = model.latent_metric(grid, columns=cols).cpu().numpy()
        share = np.trace(g[:, [qa, qb]][:, :, [qa, qb]], axis1=1, axis2=2).sum() / np.trace(g, axis1=1, axis2=2).sum()
        i, j = np.unravel_index(mag.argmax(), mag.shape)
        print('%-7s %2d dims (true blocks %s): magnification min %.3e, median %.3e, max %.3e at (x%d, x%d) = (%.2f, %.2f); '
              'share of tr G in the two grid dimensions %.3f'
              % (name, cols.size, sorted(set(block[cols].tolist())), mag.min(), np.median(mag), mag.max(), qa, qb,
                 grid[i * args.side + j, qa], grid[i * args.side + j, qb], share))
        np.save('%s_%s.npy' % (args.out, name), mag)
    np.save('%s_grid.npy' % args.out, grid[:, [qa, qb]].reshape(args.side, args.side, 2))


if __name__ == '__main__':
    main()
