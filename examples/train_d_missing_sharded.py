"""Train dp_gp_lvm (the over-D model) on data with missing entries, its D output dims sharded over the ranks of a process group,
and fill the gaps.

Launcher-agnostic: RANK / WORLD_SIZE (and MASTER_ADDR / MASTER_PORT for more than one rank) are read from the environment, as
torchrun, srun or mpirun wrappers set them; without them the script runs as a 1-rank group.  One GPU per rank (LOCAL_RANK, default
RANK modulo the visible devices), transport nccl (RCCL); --backend gloo runs several ranks on one GPU.

    torchrun --nproc_per_node 8 examples/train_d_missing_sharded.py [--iterations 300] [--seed 5] [--shard-by count]

Every rank builds the same data (same seed) and is given all of it with the full mask; it keeps its columns.  Synthetic data: D = 16
phase-shifted sines of one latent coordinate, 60 rows, 30 % of the entries removed at random.  Rank 0 prints the imputation RMSE.
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm                # noqa: E402
from dp_gp_lvm_amd.utils import missing                            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iterations', type=int, default=300)
    ap.add_argument('--seed', type=int, default=5)
    ap.add_argument('--backend', default='nccl')
    ap.add_argument('--shard-by', default='count', choices=['count', 'observed'])
    args = ap.parse_args()
    rank, world = int(os.environ.get('RANK', 0)), int(os.environ.get('WORLD_SIZE', 1))
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29511')
    device = torch.device('cuda', int(os.environ.get('LOCAL_RANK', rank)) % torch.cuda.device_count())
    torch.cuda.set_device(device)
    dist.init_process_group(args.backend, rank=rank, world_size=world)
    # the same data and the same start on every rank: q(X), Z and the atoms are replicated and must begin bit-identical
    rs = np.random.default_rng(args.seed)
    np.random.seed(args.seed)                                      # (the inducing inputs are drawn from NumPy's global generator)
    n, d, atoms = 60, 16, 3
    t = np.sort(rs.uniform(-2.5, 2.5, n))
    y = np.sin(1.3 * t[:, None] + np.pi * np.arange(d)[None, :] / d) + 0.05 * rs.standard_normal((n, d))
    y_gaps = np.where(rs.random(y.shape) >= 0.3, y, np.nan)
    mask = missing.observed_mask(y_gaps)
    model = dp_gp_lvm(y_gaps, num_latent_dims=2, num_inducing_points=10, truncation_level=atoms, observed=mask, device=device,
                      process_group=dist.group.WORLD, shard_by=args.shard_by,
                      initial_values=dict(x_var=np.full((n, 2), 0.5), gamma_atoms=np.ones((atoms, 2)),
                                          alpha_atoms=np.ones((atoms, 1)), beta_atoms=np.ones((atoms, 1))))
    before = float(model.objective)                                # (every call below is collective: all ranks make it)
    model.optimise(args.iterations, learning_rate=0.05)
    after = float(model.objective)
    imputed, var = (a.cpu().numpy() for a in model.impute_training_data(return_variance=True))      # [N x D] on every rank
    if rank == 0:
        rmse = np.sqrt(np.mean((imputed[~mask] - y[~mask]) ** 2))
        rmse_mean = np.sqrt(np.mean((missing.column_mean_filled(y_gaps, mask)[~mask] - y[~mask]) ** 2))
        print('%d rank(s); rank 0 holds columns [%d, %d) of %d' % ((world,) + tuple(model.shard) + (d,)))
        print('%d of %d entries missing' % ((~mask).sum(), mask.size))
        print('objective %.3f -> %.3f after %d iterations' % (before, after, args.iterations))
        print('imputation RMSE over the missing entries: %.4f (column means: %.4f)' % (rmse, rmse_mean))
        inside = np.abs(imputed[~mask] - y[~mask]) <= 2.0 * np.sqrt(var[~mask])
        print('%.0f %% of the missing entries lie within two predictive standard deviations' % (100.0 * inside.mean()))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
